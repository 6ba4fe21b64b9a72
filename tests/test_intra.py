"""CPU checks of the intra prediction entries: struct layouts and ABI pins, the host parameter derivation vtmhip_intra_pred_params against the Python restatement
(tests/intra_util.py) over every shape, mode and reference line, and the restatement against the recorded reference results (tests/golden/intra.npz) and, where
the reference is built, the real xPredIntraPlanar."""
import ctypes as C

import numpy as np
import pytest

import intra_util as iu
from vtm_amd import device, lib

GOLDEN = None


def golden():
    global GOLDEN
    if GOLDEN is None:
        import os
        GOLDEN = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intra.npz")))
    return GOLDEN


def golden_block(g, b):
    w, h, m, bd, off = (int(v) for v in g["blocks"][b])
    nt, nl = 2 * w + 1 + m, 2 * h + 1 + m
    return w, h, m, bd, g["lines"][off:off + nt], g["lines"][off + nt:off + nt + nl]


def test_struct_sizes_and_abi_pins():
    L = lib.load()
    for i, (s, size) in enumerate(((lib.IntraParams, 32), (lib.IntraBlock, 32), (lib.IntraJob, 16))):
        assert L.vtmhip_intra_struct_size(i) == C.sizeof(s) == size
    assert L.vtmhip_intra_struct_size(3) == -1 and L.vtmhip_intra_struct_size(-1) == -1
    assert L.vtmhip_abi_version() == 6 and L.vtmhip_struct_size(36) == -1 and L.vtmhip_sbt_struct_size(4) == -1   # the existing lists did not move
    assert C.sizeof(lib.TuJob) == 40 == L.vtmhip_struct_size(12)
    assert lib.IntraBlock.orgStride.offset == 16 and lib.IntraBlock.width.offset == 20 and lib.IntraBlock.bitDepth.offset == 24 and lib.IntraBlock.multiRefIdx.offset == 25
    assert lib.IntraJob.block.offset == 8 and lib.IntraJob.mode.offset == 12
    assert [L.vtmhip_intra_lanes_per_job(a) for a in (15, 16, 64, 65, 128, 1024, 1025, 4096, 4097)] == [0, 16, 16, 64, 64, 64, 256, 256, 0]


def test_pred_params_equal_the_restatement_everywhere():
    n = 0
    for w, h in iu.SHAPES25:
        for m in (0, 1, 2):
            for mode in range(iu.NUM_MODES):
                if mode == 0 and m:
                    continue
                p, e = device.intra_pred_params(w, h, mode, m), iu.params(w, h, mode, m)
                assert {k: getattr(p, k) for k in iu.PARAM_FIELDS} == e, (w, h, mode, m)
                n += 1
    assert n == 25 * (67 + 66 + 66)
    for bad in ((128, 8, 2, 0), (8, 2, 2, 0), (12, 8, 2, 0), (8, 8, 67, 0), (8, 8, -1, 0), (8, 8, 0, 1), (8, 8, 2, 3), (8, 8, 2, -1)):
        with pytest.raises(lib.VtmHipError):
            device.intra_pred_params(*bad)
    assert lib.load().vtmhip_intra_pred_params(8, 8, 2, 0, None) == lib.E_INVALID


def test_restatement_matches_the_recorded_reference():
    g = golden()
    assert len(g["blocks"]) >= 50 and len(g["cases"]) >= 2000
    seen = set()
    for row in g["cases"]:
        b, mode, off = int(row[0]), int(row[1]), int(row[2])
        w, h, m, bd, top, left = golden_block(g, b)
        assert dict(zip(iu.PARAM_FIELDS, (int(v) for v in row[3:]))) == iu.params(w, h, mode, m), (w, h, mode, m)
        assert np.array_equal(iu.predict(top, left, w, h, mode, m, bd), g["preds"][off:off + w * h].reshape(h, w)), (w, h, mode, m, bd)
        seen.add((w, h, m))
    assert {(w, h) for w, h, _ in seen} == set(iu.SHAPES25) and {m for _, _, m in seen} == {0, 1, 2}
    for w, h in iu.SHAPES25:       # the file holds what its recorder promises
        modes = {int(r[1]) for r in g["cases"] if tuple(g["blocks"][r[0]][:3]) == (w, h, 0)}
        assert modes == (set(range(67)) if w <= 16 and h <= 16 else set(iu.boundary_modes(w, h))), (w, h)


def test_boundary_modes_cover_the_rule_boundaries():
    for w, h in iu.SHAPES25:
        bm, par = iu.boundary_modes(w, h), {k: iu.params(w, h, k, 0) for k in range(67)}
        assert {0, 1, 2, 18, 34, 50, 66} <= set(bm)
        moved = [k for k in range(2, 67) if par[k]["predMode"] != k]
        assert (w == h) == (not moved) and all(k in bm for k in moved[:1] + moved[-1:])
        if w * h > 32:
            assert any(par[k]["refFilterFlag"] for k in bm if k > 1) and any(par[k]["interpolationFlag"] for k in bm)
            on = [bool(par[k]["refFilterFlag"] or par[k]["interpolationFlag"]) for k in bm if k > 1]
            assert True in on and (False in on or iu.INTRA_FILTER[(iu.flog2(w) + iu.flog2(h)) >> 1] == 0)


@pytest.mark.ref
def test_restatement_matches_the_real_planar(reflib):
    rng = np.random.default_rng(5)
    for w, h in iu.SHAPES25:
        for bd in (8, 10, 12):
            top, left = iu.make_lines(rng, w, h, 0, bd, "random")
            p = iu.params(w, h, 0, 0)
            t, l = iu.filter_lines(top.astype(np.int64), left.astype(np.int64)) if p["refFilterFlag"] else (top, left)
            exp = iu.ref_planar(np.asarray(t, np.int16), np.asarray(l, np.int16), w, h)
            assert np.array_equal(iu._planar(np.asarray(t, np.int64), np.asarray(l, np.int64), w, h), exp), (w, h, bd)
