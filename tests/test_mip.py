"""CPU checks of the MIP entries: struct layout and ABI pins, the Python restatement (tests/mip_util.py) against the recorded reference results
(tests/golden/mip.npz: the real prepareInputForPred / predBlock), and the host entry vtmhip_mip_pred_host against the restatement over every shape, mode,
orientation and bit depth with the recorded matrices."""
import ctypes as C

import numpy as np
import pytest

import mip_util as mu
from vtm_amd import device, lib


def test_struct_sizes_and_abi_pins():
    L = lib.load()
    assert L.vtmhip_mip_struct_size(0) == C.sizeof(lib.MipJob) == 16
    assert L.vtmhip_mip_struct_size(1) == -1 and L.vtmhip_mip_struct_size(-1) == -1
    assert lib.MipJob.block.offset == 8 and lib.MipJob.mode.offset == 12 and lib.MipJob.transposed.offset == 13
    # the existing lists did not move, and the block record is the regular modes' own
    assert L.vtmhip_abi_version() == 6 and L.vtmhip_intra_struct_size(3) == -1 and L.vtmhip_intra_struct_size(1) == C.sizeof(lib.IntraBlock) == 32
    assert [L.vtmhip_intra_lanes_per_job(a) for a in (16, 64, 65, 1024, 1025, 4096)] == [16, 16, 64, 64, 256, 256]


def test_golden_file_holds_what_its_recorder_promises():
    g = mu.golden()
    assert g["m4x4"].size == 16 * 16 * 4 and g["m8x8"].size == 8 * 16 * 8 and g["m16x16"].size == 6 * 64 * 7 and g["m4x4"].dtype == np.uint8
    assert all(np.unique(m).size > 32 for m in mu.matrices())          # trained values, not a placeholder
    seen = {}
    for blk, mode, t, _ in g["cases"]:
        w, h, bd, _ = (int(v) for v in g["blocks"][blk])
        seen.setdefault((w, h), set()).add((bd, int(mode), int(t)))
    assert set(seen) == set(mu.SHAPES25)
    for (w, h), jobs in seen.items():
        nm = mu.num_modes(w, h)
        if w <= 16 and h <= 16:
            assert jobs == {(bd, m, t) for bd in (8, 10, 12) for m in range(nm) for t in (0, 1)}, (w, h)
        else:
            assert {(m, t) for _, m, t in jobs} == {(0, 0), (0, 1), (nm - 1, 0), (nm - 1, 1)}, (w, h)
    assert {int(b[2]) for b in g["blocks"]} == {8, 10, 12}


def test_restatement_matches_the_recorded_reference():
    g = mu.golden()
    for blk, mode, t, off in (tuple(int(v) for v in r) for r in g["cases"]):
        w, h, bd, lo = (int(v) for v in g["blocks"][blk])
        top, left = g["lines"][lo:lo + w + 1], g["lines"][lo + w + 1:lo + w + h + 2]
        assert top[0] == mu.POISON and left[0] == mu.POISON
        assert np.array_equal(mu.predict(top, left, w, h, mode, t, bd), g["preds"][off:off + w * h].reshape(h, w)), (w, h, mode, t, bd)


def test_host_entry_equals_the_restatement_everywhere():
    rng, mats, n = np.random.default_rng(31), mu.matrices(), 0
    for w, h in mu.SHAPES25:
        for bd in (8, 10, 12):
            b = mu.make_mip_block(rng, w, h, bd, ("random", "alt", "random")[(bd // 2 + w + h) % 3])
            top, left = b["top"][:w + 1].copy(), b["left"][:h + 1].copy()       # exactly W + 1 and H + 1 samples
            for mode, t in mu.all_jobs(w, h):
                got = device.mip_pred_host(w, h, bd, mode, t, top, left, *mats)
                assert np.array_equal(got, mu.predict(top, left, w, h, mode, t, bd)), (w, h, mode, t, bd)
                n += 1
    assert n == 3 * 2 * (16 + 8 * 9 + 6 * 15)      # 4x4; the eight shapes with a side of 4 and 8x8; the other fifteen


def test_host_entry_rejects_what_the_device_skips():
    mats = mu.matrices()
    top, left = np.zeros(129, np.int16), np.zeros(129, np.int16)
    for bad in ((128, 8, 10, 0, 0), (8, 2, 10, 0, 0), (12, 8, 10, 0, 0), (8, 8, 7, 0, 0), (8, 8, 13, 0, 0), (4, 4, 10, 16, 0), (8, 8, 10, 8, 0), (4, 16, 10, 8, 1),
                (16, 16, 10, 6, 0), (16, 16, 10, -1, 0), (16, 16, 10, 0, 2), (16, 16, 10, 0, -1)):
        with pytest.raises(lib.VtmHipError) as e:
            device.mip_pred_host(*bad, top, left, *mats)
        assert e.value.status == lib.E_INVALID
    L, out = lib.load(), np.zeros(64, np.int16)
    ptr = [top.ctypes.data, left.ctypes.data] + [m.ctypes.data for m in mats] + [out.ctypes.data]
    assert L.vtmhip_mip_pred_host(8, 8, 10, 0, 0, *ptr) == lib.OK
    for k in range(6):
        assert L.vtmhip_mip_pred_host(8, 8, 10, 0, 0, *[None if i == k else p for i, p in enumerate(ptr)]) == lib.E_INVALID
