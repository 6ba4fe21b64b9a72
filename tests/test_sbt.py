"""CPU: the SBT part of the C ABI that needs no device (struct sizes, the host expansion, vtmhip_sbt_skip_by_rdcost), the rules against a literal table, and
the Python restatement (tests/sbt_util.py) against the recorded reference results (tests/golden/sbt.npz) and, where the reference is built, the real members."""
import ctypes as C

import numpy as np
import pytest

import sbt_util as su
from vtm_amd import device, lib

SIDES = (4, 8, 16, 32, 64)
V2, H2, V4, H4 = (1 << su.VER_HALF), (1 << su.HOR_HALF), (1 << su.VER_QUAD), (1 << su.HOR_QUAD)
# allowed mask by (side class of w, side class of h): a side of 4 allows nothing along it, 8 the half split, >= 16 half and quarter
ALLOWED = {4: (0, 0), 8: (V2, H2), 16: (V2 | V4, H2 | H4), 32: (V2 | V4, H2 | H4), 64: (V2 | V4, H2 | H4)}
D2, D8, S7 = su.DCT2, su.DCT8, su.DST7


def literal_tile(cw, ch, mode):
    """the coded rectangle (x, y, w, h) written out mode by mode"""
    return {0: (0, 0, cw // 2, ch), 1: (cw // 2, 0, cw // 2, ch), 2: (0, 0, cw, ch // 2), 3: (0, ch // 2, cw, ch // 2),
            4: (0, 0, cw // 4, ch), 5: (3 * cw // 4, 0, cw // 4, ch), 6: (0, 0, cw, ch // 4), 7: (0, 3 * ch // 4, cw, ch // 4)}[mode]


def literal_types(mode, tw, th):
    """(trHor, trVer) of the luma sub-TU written out mode by mode"""
    if mode in (0, 1, 4, 5):
        return (D2, D2) if th == 64 else {0: (D8, S7), 1: (S7, S7), 4: (D8, S7), 5: (S7, S7)}[mode]
    return (D2, D2) if tw == 64 else {2: (S7, D8), 3: (S7, S7), 6: (S7, D8), 7: (S7, S7)}[mode]


def test_struct_sizes_and_abi_pins():
    L = lib.load()
    for i, (s, size) in enumerate(((lib.SbtEstJob, 96), (lib.SbtEstResult, 280), (lib.SbtJob, 80), (lib.SbtResult, 64))):
        assert L.vtmhip_sbt_struct_size(i) == C.sizeof(s) == size and size % 8 == 0
    assert L.vtmhip_sbt_struct_size(4) == -1 and L.vtmhip_sbt_struct_size(-1) == -1
    assert L.vtmhip_abi_version() == 6 and L.vtmhip_struct_size(36) == -1   # the new structs did not move the existing list
    assert C.sizeof(lib.TuJob) == 40 == L.vtmhip_struct_size(12)
    assert (lib.SbtEstResult.rdoOrder.offset, lib.SbtEstResult.part.offset, lib.SbtEstResult.skipAll.offset) == (72, 80, 272)
    assert (lib.SbtJob.outOff.offset, lib.SbtJob.resiStride.offset, lib.SbtJob.width.offset, lib.SbtJob.qpPer.offset, lib.SbtJob.sbtIdx.offset) == (24, 48, 60, 64, 76)
    assert (lib.SBT_VER_HALF, lib.SBT_HOR_HALF, lib.SBT_VER_QUAD, lib.SBT_HOR_QUAD) == (su.VER_HALF, su.HOR_HALF, su.VER_QUAD, su.HOR_QUAD)


def _job(w, h, mode, chroma=True, bd=10):
    j = lib.SbtJob()
    j.width, j.height, j.sbtIdx, j.sbtPos, j.bitDepth, j.isIRAP = w, h, su.idx_from_mode(mode), su.pos_from_mode(mode), bd, 1
    for c in range(3):
        j.resiOff[c], j.outOff[c], j.resiStride[c], j.qpPer[c], j.qpRem[c] = (1000 * (c + 1) if c == 0 or chroma else -1), 5000 * c, 100 + c, 5 + c, c
    return j


def test_rules_against_a_literal_table():
    """Allowed masks, coded rectangles (luma and chroma) and transform pairs over every (cuW, cuH) in {4 .. 64}^2: the literal table above against the
    restatement AND against the library's own expansion (vtmhip_sbt_make_tu_jobs: sbt_rules.hpp compiled for the host)."""
    seen = 0
    for w in SIDES:
        for h in SIDES:
            mask = ALLOWED[w][0] | ALLOWED[h][1]
            assert su.sbt_allowed(w, h) == mask and su.sbt_allowed(w, h, 32) == (mask if max(w, h) <= 32 else 0)
            modes = [m for m in range(8) if (mask >> (1 + m // 2)) & 1]
            assert modes == su.allowed_modes(w, h)
            assert su.num_mode_rdo(mask) == min(2, len([m for m in modes if m < 4])) + min(2, len([m for m in modes if m >= 4]))
            for mode in range(8):
                jobs = (lib.SbtJob * 1)(_job(w, h, mode))
                if mode not in modes:
                    with pytest.raises(lib.VtmHipError):
                        device.sbt_make_tu_jobs(jobs)
                    continue
                tu, idx = device.sbt_make_tu_jobs(jobs)
                assert len(tu) == 3 and idx.tolist() == [[0, 1, 2]]
                for c in range(3):
                    cw, ch = su.comp_shape(w, h, c)
                    x, y, tw, th = literal_tile(cw, ch, mode)
                    assert su.coded_tile(cw, ch, su.idx_from_mode(mode), su.pos_from_mode(mode)) == (x, y, tw, th)
                    types = literal_types(mode, tw, th) if c == 0 else (D2, D2)
                    if c == 0:
                        assert su.tr_types(su.idx_from_mode(mode), su.pos_from_mode(mode), tw, th) == types
                    t, j = tu[c], jobs[0]
                    assert (t.resiOff, t.outOff, t.resiStride, t.width, t.height) == (j.resiOff[c] + y * j.resiStride[c] + x, j.outOff[c], j.resiStride[c], tw, th), (w, h, mode, c)
                    assert (t.typeHor, t.typeVer, t.qpPer, t.qpRem, t.bitDepth, t.isIRAP, t.pad, t.chromaAdj) == (types[0], types[1], 5 + c, c, 10, 1, 0, 0), (w, h, mode, c)
                    assert tw >= 2 and th >= 2 and (tw <= 32 or types == (D2, D2)) and (th <= 32 or types == (D2, D2))
                    seen += 1
    assert seen == 3 * sum(len(su.allowed_modes(w, h)) for w in SIDES for h in SIDES) == 3 * 140
    # mode helpers
    for idx in (1, 2, 3, 4):
        for pos in (0, 1):
            m = su.get_sbt_mode(idx, pos)
            assert m == (idx - 1) * 2 + pos and su.idx_from_mode(m) == idx and su.pos_from_mode(m) == pos
    assert [su.num_part(s) for s in SIDES] == [1, 2, 4, 4, 4]


def test_host_expansion_layout_and_argument_errors():
    jobs = (lib.SbtJob * 3)(_job(16, 16, 4), _job(8, 8, 3, chroma=False), _job(64, 32, 1))
    tu, idx = device.sbt_make_tu_jobs(jobs)
    assert len(tu) == 7 and idx.tolist() == [[0, 3, 4], [1, -1, -1], [2, 5, 6]]   # luma first, the chroma sub-TUs from n on in job order
    assert [(t.width, t.height) for t in tu] == [(4, 16), (8, 4), (32, 32), (2, 8), (2, 8), (16, 16), (16, 16)]
    L = lib.load()
    out, num = (lib.TuJob * 9)(), C.c_int(-5)
    for bad in (dict(width=12), dict(width=128), dict(height=2), dict(sbtIdx=0), dict(sbtIdx=5), dict(sbtPos=2), dict(bitDepth=7), dict(bitDepth=13)):
        j = _job(16, 16, 0)
        for k, v in bad.items():
            setattr(j, k, v)
        assert L.vtmhip_sbt_make_tu_jobs(C.addressof(j), 1, C.addressof(out), C.byref(num), None) == lib.E_INVALID, bad
    for field, c, v in (("qpRem", 0, 6), ("qpRem", 2, -1), ("qpPer", 1, -1), ("resiOff", 0, -1)):
        j = _job(16, 16, 0)
        getattr(j, field)[c] = v
        assert L.vtmhip_sbt_make_tu_jobs(C.addressof(j), 1, C.addressof(out), C.byref(num), None) == lib.E_INVALID, (field, c, v)
    j = _job(8, 16, 4)   # VER_QUAD needs a width of 16
    assert L.vtmhip_sbt_make_tu_jobs(C.addressof(j), 1, C.addressof(out), C.byref(num), None) == lib.E_INVALID
    assert num.value == -5 and L.vtmhip_sbt_make_tu_jobs(None, 0, None, C.byref(num), None) == lib.OK and num.value == 0


def _skip_inputs(seed, n):
    """est records and cost inputs spread so that every branch of skipSbtByRDCost is reached"""
    rng = np.random.default_rng(seed)
    for t in range(n):
        total = int(rng.integers(1 << 10, 1 << 34))
        est = [int(rng.integers(0, total + 1)) for _ in range(8)] + [total]
        if t % 11 == 0:
            est[int(rng.integers(0, 8))] = su.MAX_DIST
        ds = float(rng.choice([1.0 / 57.3, 0.013, 0.37, 1.0 / 3.0]))
        idx, pos = int(rng.integers(1, 5)), int(rng.integers(0, 2))
        base = ds * est[su.get_sbt_mode(idx, pos)] + (11 << 15)
        best = float(base * rng.choice([0.5, 0.999999, 1.0, 1.000001, 1.5, 4.0, 50.0]))
        dist_off = int(rng.integers(0, total + 1))
        cost_off = su.MAX_DOUBLE if t % 7 == 0 else float(ds * dist_off + rng.choice([0.0, 1000.0, 1 << 16, 1 << 20, 1 << 24]) * rng.random())
        yield est, ds, idx, pos, best, dist_off, cost_off, int(rng.integers(0, 2))


def test_skip_by_rdcost_against_the_restatement():
    seen = {}
    for args in _skip_inputs(5, 6000):
        got = device.sbt_skip_by_rdcost(*args)
        assert got == su.skip_by_rdcost(*args), args
        seen[got] = seen.get(got, 0) + 1
    assert sorted(seen) == [0, 1, 2, 3, 255] and min(seen.values()) >= 20, seen
    L = lib.load()
    e = (C.c_uint64 * 9)()
    assert L.vtmhip_sbt_skip_by_rdcost(None, 1.0, 1, 0, 1.0, 0, 1.0, 0) == lib.E_INVALID
    assert L.vtmhip_sbt_skip_by_rdcost(e, 1.0, 0, 0, 1.0, 0, 1.0, 0) == lib.E_INVALID and L.vtmhip_sbt_skip_by_rdcost(e, 1.0, 5, 0, 1.0, 0, 1.0, 0) == lib.E_INVALID
    assert L.vtmhip_sbt_skip_by_rdcost(e, 1.0, 1, 2, 1.0, 0, 1.0, 0) == lib.E_INVALID


def test_restatement_matches_the_recorded_reference():
    n, zero, coded, seen = 0, 0, 0, set()
    for g in su.golden_cases():
        idx, pos = su.idx_from_mode(g["mode"]), su.pos_from_mode(g["mode"])
        per, rem = su.qp_of(g["qp"], g["bd"])
        e = su.chain_expect(g["resi"], idx, pos, g["luma"], g["bd"], per, rem, g["irap"])
        tag = (g["w"], g["h"], g["mode"], g["luma"], g["bd"], g["qp"])
        assert np.array_equal(e["levels"], g["levels"]) and np.array_equal(e["rec_sub"], g["rec_sub"]), tag
        assert (e["sseCoded"], e["absSum"]) == (g["sse"], g["absSum"]), tag
        assert su.part_sums(g["resi"], np.zeros_like(g["resi"]), su.num_part(g["w"]), su.num_part(g["h"]), g["bd"]) == g["part"], tag
        assert sum(sum(r) for r in g["part"]) == int((g["resi"].astype(np.int64) ** 2).sum())   # distortions keep all bits at every depth
        seen.add(tag[:4])
        zero += g["absSum"] == 0
        coded += g["absSum"] > 0
        n += 1
    assert n == 152 and len(seen) == 152 and zero >= 20 and coded >= 76
    assert {g["bd"] for g in su.golden_cases()} == {8, 10, 12} and {g["qp"] for g in su.golden_cases()} == {22, 32, 42}
    # the inputs are the generator's: the file and the recipe cannot drift apart
    for (w, h, mode, luma, bd, qp, irap, r), g in zip(su.golden_case_inputs(), su.golden_cases()):
        assert (w, h, mode, luma, bd, qp, irap) == (g["w"], g["h"], g["mode"], g["luma"], g["bd"], g["qp"], g["irap"]) and np.array_equal(r, g["resi"])


def test_combination_step_on_hand_made_partitions():
    """calcMinDistSbt's combination on a 16x16 CU whose partition table is written out: the half and quad estimates, the order and the tie rule"""
    part = [[[32 * (1 + 4 * j + i) for i in range(4)] for j in range(4)], [[0] * 4 for _ in range(4)], [[0] * 4 for _ in range(4)]]
    e = su.combine(part, 16, 16, su.sbt_allowed(16, 16), 0.5, 100.0)
    d = [[32 * (1 + 4 * j + i) for i in range(4)] for j in range(4)]
    left, right = sum(d[j][i] for j in range(4) for i in (0, 1)), sum(d[j][i] for j in range(4) for i in (2, 3))
    top, bottom = sum(sum(d[j]) for j in (0, 1)), sum(sum(d[j]) for j in (2, 3))
    assert e["est"][8] == left + right == 32 * 136 and e["skipAll"] == 0
    assert e["est"][:4] == [left // 32 + right, right // 32 + left, top // 32 + bottom, bottom // 32 + top]
    col = [sum(d[j][i] for j in range(4)) for i in range(4)]
    assert e["est"][4] == col[0] // 32 + col[1] + col[2] + col[3] and e["est"][5] == col[3] // 32 + col[0] + col[1] + col[2]
    assert e["order"] == [3, 1, 7, 5, 255, 255, 255, 255]
    # a mirrored table: modes 0 / 1 and 4 / 5 tie, the lower mode comes first
    part[0] = [[10000, 7, 7, 10000]] * 4
    e = su.combine(part, 16, 16, su.sbt_allowed(16, 16), 0.5, 100.0)
    assert e["est"][0] == e["est"][1] and e["est"][4] == e["est"][5] and e["order"][:4] == [0, 1, 4, 5]
    # below the threshold nothing is estimated; a chroma sum is truncated after the weight
    assert su.combine(part, 16, 16, su.sbt_allowed(16, 16), 0.5, 1.0 / 4096)["skipAll"] == 1
    part[1][0][0] = 3
    assert su.combine(part, 16, 16, 0, 0.9, 100.0)["est"][8] == 4 * 20014 + 2


@pytest.mark.ref
def test_restatement_matches_the_real_members(reflib):
    ref = su.RefSbt(reflib)
    rng = np.random.default_rng(91)
    for idx in (1, 2, 3, 4):
        for pos in (0, 1):
            assert ref.get_sbt_mode(idx, pos) == su.get_sbt_mode(idx, pos)
    for mode in range(8):
        assert (ref.idx_from_mode(mode), ref.pos_from_mode(mode)) == (su.idx_from_mode(mode), su.pos_from_mode(mode))
    for allowed in range(32):
        assert ref.num_mode_rdo(allowed) == su.num_mode_rdo(allowed)
        for idx in (1, 2, 3, 4):
            assert ref.target_allowed(idx, allowed) == su.target_allowed(idx, allowed)
    shapes = [(w, h) for w in SIDES for h in SIDES if su.allowed_modes(w, h)]
    for t in range(160):
        w, h = shapes[t % len(shapes)]
        mode = int(rng.choice(su.allowed_modes(w, h)))
        luma, bd, qp, irap = int(rng.integers(0, 2)), int(rng.choice([8, 10, 12])), int(rng.choice([22, 27, 32, 37, 42])), int(rng.integers(0, 2))
        cw, ch = su.comp_shape(w, h, 0 if luma else 1)
        amp = int(rng.choice([1, 3, 40, (1 << bd) - 1]))
        r = rng.integers(-amp, amp + 1, (ch, cw)).astype(np.int16)
        per, rem = su.qp_of(qp, bd)
        e = su.chain_expect(r, su.idx_from_mode(mode), su.pos_from_mode(mode), luma, bd, per, rem, irap)
        g = ref.chain(r, su.idx_from_mode(mode), su.pos_from_mode(mode), luma, bd, qp, irap)
        tag = (w, h, mode, luma, bd, qp, irap, amp)
        assert np.array_equal(e["levels"], g["levels"]) and np.array_equal(e["rec"], g["rec"]) and (e["sseCoded"], e["sseZero"], e["absSum"]) == (g["sseCoded"], g["sseZero"], g["absSum"]), tag
        o = rng.integers(0, 1 << bd, (ch, cw)).astype(np.int16)
        p = rng.integers(0, 1 << bd, (ch, cw)).astype(np.int16)
        assert su.part_sums(o, p, su.num_part(w), su.num_part(h), bd) == ref.part_sums(o, p, su.num_part(w), su.num_part(h), bd), tag
