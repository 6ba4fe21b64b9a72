"""CPU: combined inter-intra prediction on the host -- vtmhip_ciip_host and vtmhip_ciip_blend_host (the rules of vtm_amd/csrc/ciip_rules.hpp) and the plain-Python
restatement of ciip_util against every case of tests/golden/ciip.npz (recorded from the reference's own predIntraAng and geneWeightedPred by
tests/golden/gen_ciip_golden.py), bit-exact; the weight rule, the size predicate, the struct sizes, the job predicate and the range of the blend."""
import ctypes as C
import os

import numpy as np
import pytest

import ciip_util as cu
import oracle_lib as ol
from vtm_amd import lib

INVALID = lib.E_INVALID


@pytest.fixture(scope="module")
def L():
    return lib.load()


@pytest.fixture(scope="module")
def golden():
    return cu.load_golden()


def test_golden_file_covers_the_issue_cases(golden):
    assert {(c["w"], c["h"]) for c in golden} == {(16, 4), (4, 16), (8, 8), (32, 8), (16, 16), (64, 64)}
    assert {(c["left_kind"], c["above_kind"]) for c in golden} == {(l, a) for l in range(3) for a in range(3)}
    assert {(c["bd"], c["kind"]) for c in golden} == {(bd, k) for bd in (8, 10, 12) for k in (0, 1)}
    assert all((c["comp"][1] is None) == (c["w"] == 4) for c in golden)
    for c in golden:
        assert c["comp"][0]["info"] == 1 | 2                                   # luma: filtered lines, PDPC, planar
        if c["comp"][1] is not None:
            # chroma: DM_CHROMA of planar is planar; no filter; PDPC unless the block is 2 high (16x4, 32x8 -> 8x2 has none, 16x4 has it)
            assert c["comp"][1]["info"] == c["comp"][2]["info"] == (2 if c["h"] >= 8 else 0)
    assert os.path.getsize(cu.GOLDEN) < 200 * 1024


def test_restatement_against_the_reference(golden):
    for c in golden:
        wi = cu.weight_intra(c["left_kind"] == 2, c["above_kind"] == 2)
        for k, p in enumerate(c["comp"]):
            if p is None:
                continue
            w, h = p["w"], p["h"]
            top, left = p["lines"][:2 * w + 1], p["lines"][2 * w + 1:]
            intra = cu.planar(top, left, w, h, filt=k == 0)
            assert np.array_equal(intra, p["intra"]), (c["w"], c["h"], k)
            assert np.array_equal(cu.blend(p["inter"], intra, wi), p["blend"]), (c["w"], c["h"], k, wi)
            if c["kind"] == 1 and k == 0:
                assert not np.array_equal(cu.planar(top, left, w, h, filt=False), p["intra"]) and not np.array_equal(cu.planar(top, left, w, h, pdpc=False), p["intra"])


def test_host_entries_against_the_reference(L, golden):
    for c in golden:
        left, above = int(c["left_kind"] == 2), int(c["above_kind"] == 2)
        p = c["comp"][0]
        w, h, bd = c["w"], c["h"], c["bd"]
        org = np.random.default_rng(w * 100 + h).integers(0, 1 << bd, (h, w)).astype(np.int16)
        job = cu.make_job(w, h, bd, [cu.make_cand(mode=cu.GIVEN, src_stride=w)], left=left, above=above)
        st, out, satd, sad = cu.host_ciip(L, job, p["lines"], org, [p["inter"]])
        assert st == 0 and np.array_equal(out[0], p["blend"]), (w, h)
        O = ol.oracle()
        mixed = np.ascontiguousarray(p["blend"])
        assert satd[0] == int(O.vo_satd(ol.P(org), w, ol.P(mixed), w, w, h)) and sad[0] == int(O.vo_sad(ol.P(org), w, ol.P(mixed), w, w, h, 0))
        assert satd[1:] == [cu.NO_COST] * 3 and sad[1:] == [cu.NO_COST] * 3
        for k in (0, 1, 2):
            q = c["comp"][k]
            if q is None:
                continue
            plane = np.full((q["h"] + 2, q["w"] + 6), 0x1234, np.int16)                     # a stride above the width; the rim stays
            plane[1:-1, 3:-3] = q["inter"]
            j = cu.blend_struct(q["w"], q["h"], bd, 0, plane.shape[1] + 3, plane.shape[1], chroma=int(k > 0), left=left, above=above)
            assert L.vtmhip_ciip_blend_host(C.byref(j), np.ascontiguousarray(q["lines"]).ctypes.data, plane.ctypes.data, None) == 0
            assert np.array_equal(plane[1:-1, 3:-3], q["blend"]), (w, h, k)
            rim = plane.copy()
            rim[1:-1, 3:-3] = 0x1234
            assert (rim == 0x1234).all()


def test_host_entry_under_lmcs_matches_the_restatement(L, golden):
    for c in golden[::5]:
        p = c["comp"][0]
        w, h, bd = c["w"], c["h"], c["bd"]
        fwd, inv = cu.make_luts(bd)
        wi = cu.weight_intra(c["left_kind"] == 2, c["above_kind"] == 2)
        rng = np.random.default_rng(7)
        org = rng.integers(0, 1 << bd, (h, w)).astype(np.int16)
        inters = [p["inter"], rng.integers(0, 1 << bd, (h, w)).astype(np.int16), p["inter"][::-1].copy()]
        job = cu.make_job(w, h, bd, [cu.make_cand(mode=m, src_stride=w, ref_stride=(w, w)) for m in (cu.GIVEN, cu.BI, cu.L1)], left=c["left_kind"] == 2,
                          above=c["above_kind"] == 2, lmcs=1)
        assert cu.host_ciip(L, job, p["lines"], org, inters)[0] == INVALID          # lmcs without the LUTs
        st, out, satd, sad = cu.host_ciip(L, job, p["lines"], org, inters, fwd, inv)
        assert st == 0
        O = ol.oracle()
        for k in range(3):
            mapped, seen = cu.candidate(inters[k], p["intra"], wi, fwd, inv)
            seen = np.ascontiguousarray(seen)
            assert np.array_equal(out[k], mapped)
            assert satd[k] == int(O.vo_satd(ol.P(org), w, ol.P(seen), w, w, h)) and sad[k] == int(O.vo_sad(ol.P(org), w, ol.P(seen), w, w, h, 0))
        assert satd[3] == sad[3] == cu.NO_COST


def test_weight_rule_over_all_flag_pairs(L):
    rng = np.random.default_rng(3)
    w, h, bd = 8, 8, 10
    lines = np.concatenate([rng.integers(0, 1024, 2 * w + 1), rng.integers(0, 1024, 2 * h + 1)]).astype(np.int16)
    lines[2 * w + 1] = lines[0]
    inter, org = rng.integers(0, 1024, (h, w)).astype(np.int16), rng.integers(0, 1024, (h, w)).astype(np.int16)
    intra = cu.planar(lines[:2 * w + 1], lines[2 * w + 1:], w, h)
    seen = {}
    for left in (0, 1):
        for above in (0, 1):
            st, out, _, _ = cu.host_ciip(L, cu.make_job(w, h, bd, [cu.make_cand(mode=cu.L0, ref_stride=(w, w))], left=left, above=above), lines, org, [inter])
            wi = cu.weight_intra(left, above)
            assert st == 0 and np.array_equal(out[0], cu.blend(inter, intra, wi))
            seen[(left, above)] = wi
    assert seen == {(0, 0): 1, (0, 1): 2, (1, 0): 2, (1, 1): 3}
    # a non-zero flag of any value counts once
    st, out, _, _ = cu.host_ciip(L, cu.make_job(w, h, bd, [cu.make_cand(ref_stride=(w, w))], left=7, above=200), lines, org, [inter])
    assert st == 0 and np.array_equal(out[0], cu.blend(inter, intra, 3))


def test_size_predicate_over_all_sides(L):
    sides = (4, 8, 16, 32, 64, 128)
    for w in sides:
        for h in sides:
            ok = w * h >= 64 and w < 128 and h < 128
            assert cu.size_ok(w, h) == ok
            if max(w, h) == 128:
                lines, org, inter = np.zeros(520, np.int16), np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
            else:
                lines, org, inter = np.zeros(2 * w + 2 * h + 2, np.int16), np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
            job = cu.make_job(w, h, 10, [cu.make_cand(ref_stride=(w, w))])
            assert (cu.host_ciip(L, job, lines, org, [inter])[0] == 0) == ok, (w, h)
    assert [cu.num_cand(n) for n in (-1, 0, 1, 2, 3, 4, 5, 6)] == [0, 0, 1, 2, 3, 4, 4, 4]


def test_job_predicate_rejects_each_malformed_field(L):
    w, h = 16, 8
    lines, org, inter = np.zeros(2 * w + 2 * h + 2, np.int16), np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
    good = lambda **kw: cu.make_job(w, h, 10, [cu.make_cand(mode=cu.BI, ref_stride=(w, w)), cu.make_cand(mode=cu.GIVEN, src_stride=w)], **kw)      # noqa: E731
    run = lambda job: cu.host_ciip(L, job, lines, org, [inter, inter, inter, inter])[0]                                                          # noqa: E731
    assert run(good()) == 0
    for bd in (7, 13):
        assert run(dict(good(), bd=bd)) == INVALID
    for n in (0, 5):
        assert run(dict(good(), num_cand=n)) == INVALID
    assert run(dict(good(), org_stride=w - 1)) == INVALID
    for field, mode in (("mode", 4), ("src_stride", w - 1)):
        job = good()
        job["cands"][1][field] = mode
        assert run(job) == INVALID
    for l in range(2):
        job = good()
        job["cands"][0]["ref_stride"][l] = w - 1
        assert run(job) == INVALID
        job["cands"][0]["mode"] = 1 - l          # the short stride belongs to the list not in use
        assert run(job) == 0
    # the blend entry: a side of 2, mapFwd on chroma, mapFwd without a LUT, a short stride
    buf = np.zeros(64 * 64, np.int16)
    for kw, ok in ((dict(w=4, h=4, chroma=1), True), (dict(w=2, h=8, chroma=1), False), (dict(w=8, h=2, chroma=1), True), (dict(w=4, h=2, chroma=1), False), (dict(w=4, h=4, chroma=0), False),
                   (dict(w=64, h=64, chroma=1), False), (dict(w=32, h=32, chroma=1), True), (dict(w=8, h=8, chroma=1, map_fwd=1), False),
                   (dict(w=8, h=8, chroma=0, map_fwd=1), False), (dict(w=8, h=8, chroma=0, stride=7), False), (dict(w=8, h=8, chroma=0, bd=13), False)):
        j = cu.blend_struct(kw["w"], kw["h"], kw.get("bd", 10), 0, 0, kw.get("stride", kw["w"]), chroma=kw["chroma"], map_fwd=kw.get("map_fwd", 0))
        assert (L.vtmhip_ciip_blend_host(C.byref(j), buf.ctypes.data, buf.ctypes.data, None) == 0) == ok, kw


def test_struct_sizes_and_abi_version(L):
    assert L.vtmhip_abi_version() == 6 and L.vtmhip_struct_size(36) == -1 and L.vtmhip_mmvd_struct_size(3) == -1      # the existing lists did not move
    assert [L.vtmhip_ciip_struct_size(i) for i in range(4)] == [C.sizeof(lib.CiipJob), C.sizeof(lib.CiipCand), C.sizeof(lib.CiipBlendJob), -1] == [288, 64, 32, -1]


@pytest.mark.parametrize("bd", [8, 12])
def test_blend_of_in_range_inputs_stays_in_range(L, bd):
    """the reference does not clip the blend: every corner of the input range, and random blocks, stay inside [0, 2^bd - 1] under every weight"""
    mx = (1 << bd) - 1
    w = h = 8
    rng = np.random.default_rng(bd)
    for lines_v in (0, mx, None):
        lines = rng.integers(0, mx + 1, 2 * w + 2 * h + 2).astype(np.int16) if lines_v is None else np.full(2 * w + 2 * h + 2, lines_v, np.int16)
        lines[2 * w + 1] = lines[0]
        for inter_v in (0, mx, None):
            inter = rng.integers(0, mx + 1, (h, w)).astype(np.int16) if inter_v is None else np.full((h, w), inter_v, np.int16)
            for left in (0, 1):
                for above in (0, 1):
                    st, out, _, _ = cu.host_ciip(L, cu.make_job(w, h, bd, [cu.make_cand(ref_stride=(w, w))], left=left, above=above), lines, inter, [inter])
                    assert st == 0 and out.min() >= 0 and out.max() <= mx
                    if lines_v is not None and inter_v is not None:
                        wi = cu.weight_intra(left, above)
                        assert (out == (((4 - wi) * inter_v + wi * lines_v + 2) >> 2)).all()
