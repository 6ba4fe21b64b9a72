"""CPU: the host side of the LFNST residual chain -- struct sizes, the mode rule against the reference's golden (tests/golden/lfnst_mode.npz: PU::getWideAngle,
TrQuant::getLFNSTIntraMode / getTransposeFlag and g_lfnstLut, all recorded from the reference's own members), and vtmhip_intra_chain_lfnst_make_jobs against a Python
restatement, with one malformed table per defect."""
import ctypes as C
import os

import numpy as np
import pytest

import lfnst_chain_util as lcu
from vtm_amd import lib
from vtm_amd.device import lfnst_mode
from vtm_amd.lib import IntraLfnstTuJob, LfnstChainJob, VtmHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = (4, 8, 16, 32, 64)


def test_struct_sizes_and_the_pins():
    L = lib.load()
    assert C.sizeof(LfnstChainJob) == 40 and C.sizeof(IntraLfnstTuJob) == 24
    assert [L.vtmhip_lfnst_chain_struct_size(k) for k in (0, 1, 2, -1)] == [40, 24, -1, -1]
    assert L.vtmhip_abi_version() == 6 and L.vtmhip_struct_size(36) == -1 and L.vtmhip_intra_chain_struct_size(2) == -1
    assert L.vtmhip_struct_size(12) == 40                                  # vtmhip_tu_job
    assert [L.vtmhip_lfnst_chain_lanes_per_job(a) for a in (16, 64, 256, 512, 4096)] == [16, 16, 16, 64, 64]


def test_mode_rule_matches_the_reference():
    z = np.load(os.path.join(ROOT, "tests", "golden", "lfnst_mode.npz"))
    lut, shapes, modes = z["lut"], z["shapes"], z["modes"]
    assert [tuple(s) for s in shapes] == [(w, h) for w in SIDES for h in SIDES] and modes.shape == (25, 67, 3)
    assert modes[:, :, 0].min() == -14 and modes[:, :, 0].max() == 80
    for s, (w, h) in enumerate(shapes):
        for mode in range(67):
            wide, set_idx, tr = (int(v) for v in modes[s, mode])
            assert lfnst_mode(int(w), int(h), mode) == (set_idx, tr), (w, h, mode)
            assert lcu.mode_of(int(w), int(h), mode, False) == (set_idx, tr)      # the restatement the other tests use
            # the recorded table itself, through the reference's index rule
            assert lut[wide + 81 if wide < 0 else wide + 14 if wide >= 67 else wide] == set_idx
        if w >= 16 and h >= 16:
            assert lfnst_mode(int(w), int(h), 33, True) == (int(lut[0]), 0) == (0, 0)
        else:
            with pytest.raises(VtmHipError):
                lfnst_mode(int(w), int(h), 0, True)
    L = lib.load()
    a, b = C.c_int(), C.c_int()
    for args in ((12, 8, 0, 0), (8, 128, 0, 0), (2, 8, 0, 0), (8, 8, 67, 0), (8, 8, -1, 0)):
        assert L.vtmhip_lfnst_mode_host(*args, C.byref(a), C.byref(b)) == lib.E_INVALID
    assert L.vtmhip_lfnst_mode_host(8, 8, 0, 0, None, C.byref(b)) == lib.E_INVALID and L.vtmhip_lfnst_mode_host(8, 8, 0, 0, C.byref(a), None) == lib.E_INVALID


# every shape class: 4x4, 8x8, a side of 4, both sides >= 8, up to 64; regular and MIP predictions; line 0 .. 2
SHAPES = [(4, 4, 0, 8, [0, 2, 66], []), (8, 8, 0, 10, [0, 1, 18, 50], [(7, 1)]), (16, 4, 1, 12, [3, 18], []), (4, 16, 2, 10, [64, 10], []), (8, 32, 0, 8, [60, 34], []),
          (16, 16, 0, 10, [0, 40], [(0, 0), (5, 1)]), (64, 64, 0, 12, [1, 66], [(3, 0)]), (64, 16, 0, 8, [5], [])]


def plain_of(p, b):
    return [(lib.DCT2, lib.DCT2, 30, p & 1)] if p % 2 == 0 else []


def lfnst_of(p, b, is_mip):
    if is_mip and min(b["w"], b["h"]) < 16:
        return []
    return [(22 + p, (p + i) & 1, i) for i in ((1, 2) if p % 3 else (2,))]


def level(order=None, shapes=SHAPES):
    rng = np.random.default_rng(11)
    lv = lcu.make_lfnst_level(rng, shapes, plain_of, lfnst_of)
    if order is not None:
        lv = lcu.LfnstLevel(lv.blocks, lv.plane, lv.tus, lv.lfnst, lfnst_order=order(lv.n_lf))
    return lv


def test_make_jobs_against_the_restatement():
    import intra_chain_util as icu
    for order in (None, lambda n: np.random.default_rng(5).permutation(n)):
        lv = level(order)
        assert lv.n_tu >= 6 and lv.n_lf >= 20 and {lv.lf_arr[k].lfnstIdx for k in range(lv.n_lf)} == {1, 2}
        assert {lv.lf_arr[k].pred >= lv.n_intra for k in range(lv.n_lf)} == {False, True}
        assert set(np.bincount([lv.tu_arr[k].pred for k in range(lv.n_tu)] + [lv.lf_arr[k].pred for k in range(lv.n_lf)])) >= {2, 3}    # plain and LFNST jobs on one prediction
        tu, lf, mw, mh, uni, lanes = lv.host_jobs()
        exp_tu, emw, emh, euni = icu.expand(lv.blk_arr, lv.intra_arr, lv.n_intra, lv.mip_arr, [lv.tu_arr[k] for k in range(lv.n_tu)])
        exp_lf, elanes = lcu.expand(lv.blk_arr, lv.intra_arr, lv.n_intra, lv.mip_arr, [lv.lf_arr[k] for k in range(lv.n_lf)])
        assert [icu.tu_fields(j) for j in tu] == exp_tu and (mw, mh, uni) == (emw, emh, euni)
        assert [lcu.chain_fields(j) for j in lf] == exp_lf and lanes == elanes == 64
        assert {(j.setIdx, j.transpose) for j in lf} >= {(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)}
    small = level(shapes=SHAPES[:4])
    assert small.host_jobs()[5] == 16 == lcu.expand(small.blk_arr, small.intra_arr, small.n_intra, small.mip_arr, [small.lf_arr[k] for k in range(small.n_lf)])[1]


def test_make_jobs_empty_tables():
    lv = level()
    no_lf = lcu.LfnstLevel(lv.blocks, lv.plane, lv.tus, [])
    tu, lf, mw, mh, uni, lanes = no_lf.host_jobs()
    assert len(tu) == lv.n_tu and len(lf) == 0 and lanes == 0 and (mw, mh) == (64, 64)
    no_tu = lcu.LfnstLevel(lv.blocks, lv.plane, [], lv.lfnst)
    tu, lf, mw, mh, uni, lanes = no_tu.host_jobs()
    assert len(tu) == 0 and len(lf) == lv.n_lf and (mw, mh, uni, lanes) == (0, 0, 0, 64)
    L = lib.load()
    assert L.vtmhip_intra_chain_lfnst_make_jobs(None, 0, None, 0, None, 0, None, 0, None, 0, None, None, None, None, None, None) == lib.OK
    assert L.vtmhip_intra_chain_lfnst_make_jobs(None, 0, None, 0, None, 0, None, 0, None, -1, None, None, None, None, None, None) == lib.E_INVALID
    assert L.vtmhip_intra_chain_lfnst_make_jobs(C.addressof(lv.blk_arr), len(lv.blocks), C.addressof(lv.intra_arr), lv.n_intra, C.addressof(lv.mip_arr), lv.n_mip, None, 0,
                                                C.addressof(lv.lf_arr), lv.n_lf, None, None, None, None, None, None) == lib.E_INVALID      # LFNST jobs without an output


def _lf(k, field, v, idx=None):
    def f(lv):
        if idx is None:
            setattr(lv.lf_arr[k], field, v)
        else:
            getattr(lv.lf_arr[k], field)[idx] = v
    return f


def _mip_on_8x8(lv):
    lv.lf_arr[0].pred = lv.n_intra            # MIP job 0 sits on the 8x8 block


def _blk(k, field, v):
    return lambda lv: setattr(lv.blk_arr[k], field, v)


DEFECTS = [("lfnstIdx 0", _lf(1, "lfnstIdx", 0)), ("lfnstIdx 3", _lf(1, "lfnstIdx", 3)), ("MIP on a block with a side below 16", _mip_on_8x8),
           ("pred past both tables", _lf(2, "pred", 10 ** 6)), ("pred -1", _lf(2, "pred", -1)), ("qpRem 6", _lf(3, "qpRem", 6)), ("qpPer -1", _lf(3, "qpPer", -1)),
           ("reserved[0]", _lf(4, "reserved", 1, 0)), ("reserved[1]", _lf(4, "reserved", 1, 1)), ("pad", _lf(4, "pad", 1)), ("block width 12", _blk(2, "width", 12)),
           ("block bitDepth 13", _blk(0, "bitDepth", 13))]


@pytest.mark.parametrize("name,defect", DEFECTS, ids=[n for n, _ in DEFECTS])
def test_a_malformed_table_is_rejected_and_out_untouched(name, defect):
    lv = level()
    defect(lv)
    L = lib.load()
    out_tu, out_lf = np.full(40 * lv.n_tu, 0xa5, np.uint8), np.full(40 * lv.n_lf, 0xa5, np.uint8)
    lanes = C.c_int(-7)
    st = L.vtmhip_intra_chain_lfnst_make_jobs(C.addressof(lv.blk_arr), len(lv.blocks), C.addressof(lv.intra_arr), lv.n_intra, C.addressof(lv.mip_arr), lv.n_mip,
                                              C.addressof(lv.tu_arr), lv.n_tu, C.addressof(lv.lf_arr), lv.n_lf, out_tu.ctypes.data, out_lf.ctypes.data, None, None, None,
                                              C.byref(lanes))
    assert st == lib.E_INVALID and (out_tu == 0xa5).all() and (out_lf == 0xa5).all() and lanes.value == -7
