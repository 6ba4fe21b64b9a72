"""CPU: the LMCS part of the C ABI that needs no device (struct sizes, the job layouts that carry chromaAdj) and the numpy restatement of the
reference's rules (tests/lmcs_util.py) against the recorded reference results (tests/golden/lmcs.npz), Python integers and, where the reference is
built, the real members."""
import ctypes as C

import numpy as np
import pytest

import lmcs_util as lu
from vtm_amd import lib

EDGE_VALUES, EDGE_SCALES = lu.EDGE_VALUES, lu.EDGE_SCALES


def test_struct_sizes_and_abi_pins():
    L = lib.load()
    for i, (s, size) in enumerate(((lib.LmcsJob, 56), (lib.ScaleJob, 32))):
        assert L.vtmhip_lmcs_struct_size(i) == C.sizeof(s) == size and size % 8 == 0
    assert L.vtmhip_lmcs_struct_size(2) == -1 and L.vtmhip_lmcs_struct_size(-1) == -1
    # the jobs that carry chromaAdj kept their size and every existing field its place
    assert C.sizeof(lib.TuJob) == 40 == L.vtmhip_struct_size(12) and C.sizeof(lib.JccrJob) == 48 == L.vtmhip_jccr_struct_size(1)
    tu = {f: getattr(lib.TuJob, f).offset for f in ("resiOff", "outOff", "resiStride", "width", "height", "qpPer", "qpRem", "typeHor", "typeVer", "bitDepth", "isIRAP", "pad")}
    assert tu == dict(resiOff=0, outOff=8, resiStride=16, width=20, height=22, qpPer=24, qpRem=26, typeHor=28, typeVer=29, bitDepth=30, isIRAP=31, pad=32)
    assert lib.TuJob.chromaAdj.offset == 36 and lib.TuJob.chromaAdj.size == 4
    jc = {f: getattr(lib.JccrJob, f).offset for f in ("cbOff", "crOff", "outOff", "resiStride", "width", "height", "qpPer", "qpRem", "typeHor", "bitDepth", "isIRAP",
                                                      "cbfMask", "signFlag", "pad")}
    assert jc == dict(cbOff=0, crOff=8, outOff=16, resiStride=24, width=28, height=30, qpPer=32, qpRem=34, typeHor=36, bitDepth=37, isIRAP=38, cbfMask=39, signFlag=40, pad=41)
    assert lib.JccrJob.chromaAdj.offset == 42 and lib.JccrJob.chromaAdj.size == 2 and C.sizeof(lib.JccrJob().pad) == 7
    j = lib.JccrJob()
    j.chromaAdj = 0x1234
    assert bytes(j)[40:48] == bytes([0, 0, 0x34, 0x12, 0, 0, 0, 0]) and list(j.pad) == [0, 0x34, 0x12, 0, 0, 0, 0]
    assert L.vtmhip_abi_version() == 6 and L.vtmhip_struct_size(36) == -1   # the new structs did not move the existing list
    assert (lib.LMCS_MAP_PRED, lib.LMCS_WRITE_MAPPED) == (lu.MAP_PRED, lu.WRITE_MAPPED)


def test_restatement_matches_the_recorded_reference():
    n, sat, clip_in, clip16, seen = 0, 0, 0, 0, set()
    for w, h, bd, fwd, scale, blk, out in lu.golden_scale_cases():
        assert np.array_equal(lu.scale_signal(blk, scale, fwd, bd), out), (w, h, bd, fwd, scale)
        m = (1 << bd) - 1
        if fwd:
            sat += int(lu.saturated(blk, scale, bd).any())
        else:
            clip_in += int(((blk > m) | (blk < -m - 1)).any())
            clip16 += int((np.abs(np.clip(blk.astype(np.int64), -m - 1, m)) * scale + 1024 >> 11 > 32767).any())
        seen.add((w, h, bd, fwd, scale))
        n += 1
    assert n == 972 and len(seen) == 6 * 3 * 2 * 9 and sat > 0 and clip_in > 0 and clip16 > 0   # the file holds every clip of the two rules
    # the inputs are the generator's: the file and the recipe cannot drift apart
    for (w, h, bd, fwd, scale, blk), (_w, _h, _bd, _f, _s, rec_in, _o) in zip(lu.golden_case_inputs(), lu.golden_scale_cases()):
        assert (w, h, bd, fwd, scale) == (_w, _h, _bd, _f, _s) and np.array_equal(blk, rec_in)
    z = lu.golden()
    for k in range(len(z["rsp_w"])):
        w, h, bd, o = int(z["rsp_w"][k]), int(z["rsp_h"][k]), int(z["rsp_bd"][k]), int(z["rsp_off"][k])
        lut = z["rsp_lut"][(bd - 8) // 2][:1 << bd]
        assert np.array_equal(lut, lu.make_lut(100 + bd, bd))
        mapped = lu.rsp_signal(z["rsp_in"][o:o + w * h], lut)
        assert np.array_equal(mapped, z["rsp_out"][o:o + w * h])
        assert np.array_equal(lu.reco_expect(mapped, z["rsp_resi"][o:o + w * h], lut, False, bd), z["rsp_reco"][o:o + w * h])


def test_scale_2048_is_not_a_no_op_on_the_inverse_side():
    blk = np.array([[5000, -5000, 1023, -1024]], np.int16)
    assert lu.scale_signal(blk, 2048, 0, 10).tolist() == [[1023, -1024, 1023, -1024]]
    assert lu.scale_signal(blk, 2048, 1, 10).tolist() == [[1023, -1023, 1023, -1023]]


def test_division_of_the_restatement_is_exact():
    """The forward rule against Python integers: every scale 1 .. 32767 against the edge values, and every |v| <= 4095 against the edge scales."""
    for bd in (8, 12):
        m = (1 << bd) - 1
        vals = np.array([v for v in EDGE_VALUES if v <= 32767] + [-v for v in EDGE_VALUES], np.int64)
        for scale in list(range(1, 32768, 97)) + EDGE_SCALES:
            got = lu.scale_signal(vals.astype(np.int16), scale, 1, bd).tolist()
            exp = [max(-m, min(m, (1 if v >= 0 else -1) * (((abs(v) << 11) + (scale >> 1)) // scale))) for v in vals.astype(np.int16).tolist()]
            assert got == exp, (bd, scale)
    allv = np.arange(-4095, 4096, dtype=np.int16)
    for scale in EDGE_SCALES:
        got = lu.scale_signal(allv, scale, 1, 12).tolist()
        exp = [max(-4095, min(4095, (1 if v >= 0 else -1) * (((abs(v) << 11) + (scale >> 1)) // scale))) for v in allv.tolist()]
        assert got == exp, scale
        inv = lu.scale_signal(allv, scale, 0, 12).tolist()
        expi = [max(-32768, min(32767, (1 if v >= 0 else -1) * ((abs(v) * scale + 1024) >> 11))) for v in allv.tolist()]
        assert inv == expi, scale


def test_the_reciprocal_of_the_device_rule_is_exact():
    """vtm_amd/csrc/lmcs.hpp divides with magic = floor((2^32 - 1) / scale), q0 = (N * magic) >> 32 and one conditional increment.  Its argument (q0 is the
    quotient or one below it for N < 2^27) checked in Python integers at the largest numerators and around every multiple of the scale near them."""
    for scale in list(range(1, 32768, 61)) + EDGE_SCALES:
        magic = 0xffffffff // scale
        tops = [(32768 << 11) + (scale >> 1), (32767 << 11) + (scale >> 1), (4095 << 11) + (scale >> 1)]
        ns = set(tops)
        for t in tops:
            k = t // scale
            ns.update(n for n in (k * scale - 1, k * scale, k * scale + 1, (k - 1) * scale, (k - 1) * scale + scale - 1) if 0 <= n <= tops[0])
        ns.update((0, 1, scale - 1, scale, scale + 1))
        for n in ns:
            q0 = (n * magic) >> 32
            assert q0 in (n // scale, n // scale - 1), (scale, n)
            q = q0 + (1 if n - q0 * scale >= scale else 0)
            assert q == n // scale, (scale, n)


@pytest.mark.ref
def test_restatement_matches_the_real_members(reflib):
    ref = lu.RefLmcs(reflib)
    rng = np.random.default_rng(78)
    for t in range(1500):
        w, h = int(rng.choice([2, 4, 8, 16])), int(rng.choice([1, 2, 4, 8, 16]))
        bd, fwd = int(rng.choice([8, 10, 12])), t % 2
        scale = int(rng.choice(EDGE_SCALES)) if t % 3 else int(rng.integers(1, 32768))
        amp = int(rng.choice([3, 200, (1 << bd) - 1, 32767]))
        blk = rng.integers(max(-amp, -32768), amp + 1, (h, w)).astype(np.int16)
        if amp == 32767:
            blk[0, 0], blk[h - 1, w - 1] = -32768, 32767
        assert np.array_equal(lu.scale_signal(blk, scale, fwd, bd), ref.scale_signal(blk, scale, fwd, bd)), (w, h, bd, fwd, scale, amp)
    for bd in (8, 10, 12):
        lut = lu.make_lut(bd, bd)
        blk = rng.integers(0, 1 << bd, (12, 20)).astype(np.int16)
        resi = rng.integers(-(1 << bd), 1 << bd, (12, 20)).astype(np.int16)
        mapped = ref.rsp_signal(blk, lut)
        assert np.array_equal(mapped, lu.rsp_signal(blk, lut))
        assert np.array_equal(ref.reconstruct(mapped, resi, bd), lu.reco_expect(blk, resi, lut, True, bd))
