"""CPU: the JCCR / ICT part of the C ABI that needs no device (struct sizes, vtmhip_ict_select) and the numpy restatement of the reference's rules
(tests/jccr_util.py) against the recorded reference results (tests/golden/jccr.npz) and, where the reference is built, the real templates."""
import ctypes as C
import itertools

import numpy as np
import pytest

import jccr_util as ju
from vtm_amd import lib
from vtm_amd.device import ict_select


def test_struct_sizes_and_abi_pins():
    L = lib.load()
    for i, (s, size) in enumerate(((lib.IctJob, 40), (lib.JccrJob, 48), (lib.JccrResult, 32))):
        assert L.vtmhip_jccr_struct_size(i) == C.sizeof(s) == size and size % 8 == 0
    assert L.vtmhip_jccr_struct_size(3) == -1 and L.vtmhip_jccr_struct_size(-1) == -1
    assert L.vtmhip_abi_version() == 6 and L.vtmhip_struct_size(36) == -1   # the new structs did not move the existing list
    assert lib.ICT_MODES == ju.ICT_MODES


def _check_select(dist):
    for intra in (0, 1):
        assert ict_select(dist, intra) == ju.select_ict(dist, intra), (dist, intra)


def test_ict_select_matches_the_rule():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        hi = int(rng.choice([10, 1000, 1 << 20, 1 << 40]))
        _check_select([[int(v) for v in rng.integers(0, hi, 2)] for _ in range(4)])
    # every ordering of four small distances (the plain candidate's distance is min(d1, d2) of pair 0), ties included
    for d in itertools.product(range(4), repeat=4):
        _check_select([[d[0] * 8, 1000], [d[1] * 8, 0], [d[2] * 8, 0], [d[3] * 8, 0]])
        _check_select([[1000, d[0] * 8], [d[1] * 8, 0], [d[2] * 8, 0], [d[3] * 8, 0]])
    # the thresholds: second best exactly at, one below and one above 9 * min / 8 (a mask won) and 3 * min / 2 (no mask won)
    for mn in (8, 64, 80, 801, 12345):
        for delta in (-1, 0, 1):
            for first, second in itertools.permutations((1, 2, 3), 2):
                d = [[10 ** 9, 10 ** 9], [10 ** 8, 0], [10 ** 8, 0], [10 ** 8, 0]]
                d[first][0], d[second][0] = mn, 9 * mn // 8 + delta
                _check_select(d)
            for second in (1, 2, 3):
                d = [[mn, 10 ** 9], [10 ** 8, 0], [10 ** 8, 0], [10 ** 8, 0]]
                d[second][0] = 3 * mn // 2 + delta
                _check_select(d)
    assert ict_select([[5, 9], [1, 0], [2, 0], [3, 0]], 0) == [3]
    assert ict_select([[80, 90], [70, 0], [77, 0], [79, 0]], 1) == [1, 2]
    assert ict_select([[80, 90], [70, 0], [78, 0], [79, 0]], 1) == [1]        # 9 * 70 / 8 is 78 in integers (78.75 exactly): 78 is not below it
    L = lib.load()
    assert L.vtmhip_ict_select(None, 1, (C.c_int * 2)(), C.byref(C.c_int())) == lib.E_INVALID


def test_restatement_matches_the_recorded_reference():
    n, modes, wraps, clips = 0, set(), 0, 0
    for m, cb, cr, joint, dist, inv in ju.golden_cases():
        j, d = ju.fwd_ict(m, cb, cr)
        assert d == dist, (m, cb.shape)
        if m:
            assert np.array_equal(j, joint), (m, cb.shape)
            am, s = abs(m), (-1 if m < 0 else 1)
            exact = (4 * cb.astype(np.int64) + s * 2 * cr) if am == 1 else (cb.astype(np.int64) + s * cr) if am == 2 else (4 * cr.astype(np.int64) + s * 2 * cb)
            wraps += int((np.abs(exact) // (2 if am == 2 else 5) > 32767).any())
        icb, icr = ju.inv_ict(m, cb, cr)
        assert np.array_equal(icb if abs(m) == 3 else icr, inv), ("inv", m, cb.shape)
        clips += int(m == -2 and (cb == -32768).any())
        n += 1
        modes.add(m)
    assert n >= 200 and modes == set(ju.MODES) and wraps > 0 and clips > 0   # the file holds Pel wraps and the -32768 clip


@pytest.mark.ref
def test_restatement_matches_the_real_templates(reflib):
    ref = ju.RefICT(reflib)
    rng = np.random.default_rng(77)
    for t in range(1400):
        m = ju.MODES[t % 7]
        w, h = int(rng.choice([2, 4, 8, 16])), int(rng.choice([2, 4, 8, 16]))
        amp = int(rng.choice([3, 200, 1023, 4095, 32767]))
        cb, cr = ju.random_pair(rng, w, h, amp, full_range=amp == 32767)
        if m == -2 and t % 3 == 0:
            cb[0, 0] = -32768
        j, d = ju.fwd_ict(m, cb, cr)
        rj, rd = ref.fwd_ict(m, cb, cr)
        assert d == rd and (m == 0 or np.array_equal(j, rj)), (m, w, h, amp)
        a, b = ju.inv_ict(m, cb, cr)
        ra, rb = ref.inv_ict(m, cb, cr)
        assert np.array_equal(a, ra) and np.array_equal(b, rb), ("inv", m, w, h, amp)
