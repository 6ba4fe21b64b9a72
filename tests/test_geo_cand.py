"""CPU: the GEO merge estimation on the host -- the rules of vtm_amd/csrc/geo_rules.hpp through vtmhip_geo_tables_host and vtmhip_geo_host against
tests/golden/geo_cand.npz (recorded from the reference's own tables, RdCost, GeoComboCostList and xWeightedGeoBlk by tests/golden/gen_geo_cand_golden.py) and against
the weight planes of tests/golden/geo.npz read with the reference's address arithmetic, bit-exact; the tie order, the predicate and the struct sizes."""
import ctypes as C
import os

import numpy as np
import pytest

import geo_util as gu
from vtm_amd import lib

INVALID = lib.E_INVALID


@pytest.fixture(scope="module")
def L():
    return lib.load()


@pytest.fixture(scope="module")
def golden():
    return gu.load_golden()


def tables(L, split, w, h, chroma):
    wt, mk = np.zeros((h >> chroma, w >> chroma), np.int16), np.zeros((h, w), np.int16)
    assert L.vtmhip_geo_tables_host(split, w, h, chroma, wt.ctypes.data, mk.ctypes.data) == 0
    return wt, mk


def test_golden_file_covers_the_issue_cases(golden):
    cases = golden["cases"]
    assert {(c["w"], c["h"]) for c in cases} == {(8, 8), (16, 8), (8, 16), (32, 32), (64, 16), (16, 64), (64, 64)}
    assert {c["bd"] for c in cases} == {8, 10, 12} and {c["num_cand"] for c in cases} == {2, 3, 6}
    assert any(c["num_passed"] == 0 for c in cases) and any(0 < c["num_passed"] < 60 for c in cases) and any(c["num_passed"] > 60 for c in cases)
    for c in cases:                                                  # the tie condition of the recording (the 61st cost is not kept: the generator asserts it)
        assert len(set(c["cost"].tolist())) == len(c["cost"])
    assert os.path.getsize(gu.GOLDEN) < 512 * 1024


def test_tables_and_offsets_against_the_reference(L, golden):
    assert golden["params"].tolist() == [list(p) for p in gu.SPLITS] and len(gu.SPLITS) == 64
    assert [tuple(p) for p in golden["order"].tolist()] == gu.PAIRS
    for s in range(64):
        for hi in range(4):
            for wi in range(4):
                assert tuple(golden["offsets"][s, hi, wi].tolist()) == gu.weight_offset(s, 8 << wi, 8 << hi), (s, wi, hi)
    # the library's statement of the same tables, seen through its outputs: the plane entry at the recorded offset (mirror 0 splits read it unmirrored)
    planes = gu.weight_planes()
    for s, (a, d) in enumerate(gu.SPLITS):
        if gu.ANGLE2MIRROR[a]:
            continue
        for w, h in gu.SHAPES:
            ox, oy = golden["offsets"][s, h.bit_length() - 4, w.bit_length() - 4].tolist()
            wt, _ = tables(L, s, w, h, 0)
            assert np.array_equal(wt, planes[gu.ANGLE2MASK[a]][oy:oy + h, ox:ox + w]), (s, w, h)


def test_tables_host_against_the_planes(L):
    """every (shape, split, luma / chroma): the weights against the recorded g_globalGeoWeights planes and the mask against the mask planes, both read with the
    reference's address arithmetic (blend_walk / sad_walk); all three mirror cases and both offset branches occur"""
    planes, masks = gu.weight_planes(), gu.mask_planes()
    seen_mirror, seen_branch = set(), set()
    for w, h in gu.SHAPES:
        for s in range(64):
            a, d = gu.SPLITS[s]
            seen_mirror.add(gu.ANGLE2MIRROR[a])
            if d > 0:
                seen_branch.add(a % 16 == 8 or (a % 16 != 0 and h >= w))
            for chroma in (0, 1):
                wt, mk = tables(L, s, w, h, chroma)
                mi, first, sx, row = gu.blend_walk(s, w, h, chroma)
                assert np.array_equal(wt, gu.plane_block(planes[mi], first, sx, row, w >> chroma, h >> chroma)), (w, h, s, chroma)
                mi, first, ms, stx, ms2 = gu.sad_walk(s, w, h)
                assert np.array_equal(mk, gu.plane_block(masks[mi], first, stx, w * stx + ms + ms2, w, h)), (w, h, s)
    assert seen_mirror == {0, 1, 2} and seen_branch == {True, False}
    assert L.vtmhip_geo_tables_host(64, 8, 8, 0, None, None) == INVALID and L.vtmhip_geo_tables_host(0, 64, 8, 0, None, None) == INVALID
    assert L.vtmhip_geo_tables_host(0, 8, 8, 0, None, None) == 0


def test_mask_is_positive_weight_index():
    """the planes themselves: the recorded weight planes are Clip3( 0, 8, ( 32 + wIdx + 4 ) >> 3 ) of the wIdx written out here, geo_util's mask planes are wIdx > 0
    of the same wIdx, and the two agree wherever the weight decides the sign (a weight of 4 is wIdx in -4 .. 3)"""
    planes, masks = gu.weight_planes(), gu.mask_planes()
    yy, xx = np.mgrid[0:gu.M, 0:gu.M]
    for a in range(9):
        mi = gu.ANGLE2MASK[a]
        if mi < 0:
            continue
        dx, dy = gu.DIS[a], gu.DIS[(a + 8) % 32]
        idx = (2 * (xx + 8) + 1) * dx + (2 * (yy + 8) + 1) * dy - ((dx + dy) << 7)
        assert np.array_equal(planes[mi], ((32 + idx + 4) >> 3).clip(0, 8))
        assert np.array_equal(masks[mi], idx > 0)
        assert np.all(masks[mi][planes[mi] > 4] == 1) and np.all(masks[mi][planes[mi] < 4] == 0)


def test_mask_on_all_shapes(L):
    """mask == (wIdx > 0) and weight == Clip3( 0, 8, ( 32 + wIdx + 4 ) >> 3 ), exactly, on all 14 shapes and 64 splits: wIdx is written out here per plane entry, and
    the entry of a sample is the one the masked SAD's set-up walks to"""
    yy, xx = np.mgrid[0:gu.M, 0:gu.M]
    widx = {}
    for a in range(9):
        if gu.ANGLE2MASK[a] >= 0:
            dx, dy = gu.DIS[a], gu.DIS[(a + 8) % 32]
            widx[gu.ANGLE2MASK[a]] = (2 * (xx + 8) + 1) * dx + (2 * (yy + 8) + 1) * dy - ((dx + dy) << 7)
    assert sorted(widx) == list(range(6))
    for w, h in gu.SHAPES:
        for s in range(64):
            wt, mk = tables(L, s, w, h, 0)
            mi, first, ms, stx, ms2 = gu.sad_walk(s, w, h)
            idx = gu.plane_block(widx[mi], first, stx, w * stx + ms + ms2, w, h)
            assert np.array_equal(mk, (idx > 0).astype(np.int16)), (w, h, s)
            assert np.array_equal(wt, ((32 + idx + 4) >> 3).clip(0, 8)), (w, h, s)
            assert 0 < mk.sum() < w * h


def test_host_entry_against_the_reference(L, golden):
    for c in golden["cases"]:
        w, h, bd, nc = c["w"], c["h"], c["bd"], c["num_cand"]
        for use_satd in (1, 0):
            st, res, split, blend = gu.host_job(L, gu.geo_job(w, h, bd, nc, c["lam"]), c["org"], c["pred"], use_satd)
            assert st == 0
            assert list(res.sadWhole) == c["sad_whole"].tolist(), (w, h, bd)
            assert np.array_equal(split, c["sad_large"]), (w, h, bd)
            nt = min(c["num_passed"], 60)
            assert (res.numPassed, res.numTested) == (c["num_passed"], nt)
            rows = gu.result_rows(res)
            exp = [(int(s), int(a), int(b), np.float64(cost).view(np.uint64).item(), int(d[0 if use_satd else 1])) for (s, a, b), cost, d in zip(c["list"], c["cost"], c["dist"])]
            assert rows[:nt] == exp, (w, h, bd, nc)
            assert all(r == (0, 0, 0, 0, gu.NO_COST) for r in rows[nt:])
            assert np.array_equal(blend[:len(c["blend"])], c["blend"]), (w, h, bd)


def test_chroma_weights_against_the_reference(L, golden):
    n = 0
    for c in golden["cases"]:
        for ch in c["chroma"]:
            wt, _ = tables(L, ch["split"], c["w"], c["h"], 1)
            bd = c["bd"]
            shift = max(2, 14 - bd) + 3
            v = (wt.astype(np.int64) * ch["src0"] + (8 - wt.astype(np.int64)) * ch["src1"] + (1 << (shift - 1)) + (8192 << 3)) >> shift
            assert np.array_equal(v.clip(0, (1 << bd) - 1), ch["blend"]), (c["w"], c["h"], ch["split"], ch["comp"])
            n += 1
    assert n >= 40


def test_ties_come_out_in_the_stated_order(L):
    """duplicate candidates make equal costs: splitDir first, then the index in the pair order"""
    rng = np.random.default_rng(5)
    w, h, bd = 16, 8, 10
    org = rng.integers(0, 1024, (h, w)).astype(np.int16)
    a = ((rng.integers(0, 1024, (h, w)) << 4) - 8192).astype(np.int16)
    st, res, split, _ = gu.host_job(L, gu.geo_job(w, h, bd, 3, 0.0), org, [a, a, a])
    assert st == 0 and res.numPassed == 64 * 6 and res.numTested == 60                       # lambda 0: every combination costs the whole SAD
    rows = gu.result_rows(res)
    assert [(r[0], r[1], r[2]) for r in rows] == [(t // 6,) + gu.PAIRS[t % 6] for t in range(60)]
    assert len({r[3] for r in rows}) == 1
    # two equal candidates among three, a lambda that is no dyadic fraction: the pairs (0, 1) / (1, 0) differ in their bits, (0, 2) / (1, 2) tie in SAD only
    b = ((rng.integers(0, 1024, (h, w)) << 4) - 8192).astype(np.int16)
    st, res, split, _ = gu.host_job(L, gu.geo_job(w, h, bd, 3, 0.1), org, [a, a, b])
    assert st == 0
    rows = gu.result_rows(res)[:res.numTested]
    keys = [(r[3], r[0], gu.PAIRS.index((r[1], r[2]))) for r in rows]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_predicate(L):
    rng = np.random.default_rng(1)
    org = rng.integers(0, 1024, (8, 8)).astype(np.int16)
    p = [((rng.integers(0, 1024, (8, 8)) << 4) - 8192).astype(np.int16) for _ in range(6)]

    def status(**kw):
        j = gu.geo_job(8, 8, 10, 2, 1.0)
        for k, v in kw.items():
            if k == "ref_stride1":
                j.cand[1].refStride = v
            else:
                setattr(j, k, v)
        return gu.host_job(L, j, org, p)[0]

    assert status() == 0 and status(numCand=6) == 0 and status(bitDepth=8) == 0 and status(bitDepth=12) == 0 and status(sqrtLambda=0.0) == 0
    for bad in (dict(width=4), dict(width=64), dict(height=12), dict(height=128), dict(bitDepth=7), dict(bitDepth=13), dict(numCand=1), dict(numCand=7),
                dict(orgStride=7), dict(ref_stride1=7), dict(sqrtLambda=-0.5), dict(sqrtLambda=float("inf")), dict(sqrtLambda=float("nan"))):
        assert status(**bad) == INVALID, bad
    assert sum(1 for w in (8, 16, 32, 64) for h in (8, 16, 32, 64) if gu.host_job(L, gu.geo_job(w, h, 10, 2, 1.0), np.zeros((h, w), np.int16),
                                                                                  [np.zeros((h, w), np.int16)] * 2, want_blend=False)[0] == 0) == 14


def test_struct_sizes_and_lanes(L):
    assert [L.vtmhip_geo_struct_size(i) for i in range(6)] == [C.sizeof(lib.GeoJob), C.sizeof(lib.GeoCand), C.sizeof(lib.GeoCombo), C.sizeof(lib.GeoResult),
                                                              C.sizeof(lib.GeoCuBlendJob), -1]
    assert (C.sizeof(lib.GeoJob), C.sizeof(lib.GeoCand), C.sizeof(lib.GeoCombo), C.sizeof(lib.GeoResult), C.sizeof(lib.GeoCuBlendJob)) == (224, 32, 24, 1496, 48)
    assert L.vtmhip_struct_size(36) == -1 and L.vtmhip_abi_version() == 6
    assert {(w, h): L.vtmhip_geo_lanes_per_job(w, h) for w, h in gu.SHAPES} == {(w, h): 64 if w * h <= 1024 else 256 for w, h in gu.SHAPES}
    assert L.vtmhip_geo_lanes_per_job(64, 8) == 0 and L.vtmhip_geo_lanes_per_job(4, 4) == 0 and L.vtmhip_geo_lanes_per_job(128, 128) == 0
