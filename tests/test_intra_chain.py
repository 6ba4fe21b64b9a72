"""CPU: the tables of the intra residual chain.  Struct layouts, the pins that must not move, vtmhip_intra_chain_make_tu_jobs (the host form of the entry's checks
and expansion) against a Python restatement on a mixed table, and every rejection -- one table per defect."""
import ctypes as C

import numpy as np
import pytest

import intra_chain_util as icu
from vtm_amd import lib
from vtm_amd.device import intra_chain_make_tu_jobs
from vtm_amd.lib import IntraTuJob, IntraTuResult, TuJob, VtmHipError


def test_struct_sizes_and_the_pins_that_must_not_move():
    L = lib.load()
    assert C.sizeof(IntraTuJob) == 24 and C.sizeof(IntraTuResult) == 24
    assert L.vtmhip_intra_chain_struct_size(0) == 24 and L.vtmhip_intra_chain_struct_size(1) == 24
    assert L.vtmhip_intra_chain_struct_size(2) == -1 and L.vtmhip_intra_chain_struct_size(-1) == -1
    assert L.vtmhip_abi_version() == 6 and L.vtmhip_struct_size(36) == -1 and L.vtmhip_intra_struct_size(3) == -1 and L.vtmhip_mip_struct_size(1) == -1
    assert C.sizeof(TuJob) == 40


def _call(lv):
    return intra_chain_make_tu_jobs(lv.blk_arr if lv.blocks else None, lv.intra_arr if lv.n_intra else None, lv.mip_arr if lv.n_mip else None,
                                    lv.tu_arr if lv.n_tu else None)


def _same(lv):
    got, mw, mh, uni = _call(lv)
    exp, emw, emh, euni = icu.expand(lv.blk_arr, lv.intra_arr, lv.n_intra, lv.mip_arr, [lv.tu_arr[k] for k in range(lv.n_tu)])
    assert len(got) == lv.n_tu and [icu.tu_fields(j) for j in got] == exp
    assert (mw, mh, uni) == (emw, emh, euni)
    return mw, mh, uni


def test_expansion_of_a_mixed_table():
    rng = np.random.default_rng(41)
    cands = [(lib.DCT2, lib.DCT2), (lib.DST7, lib.DST7), (lib.DCT8, lib.DST7), (lib.TRSKIP, lib.TRSKIP)]

    def tus_of(p, b):
        n = 1 + p % 4 if max(b["w"], b["h"]) <= 32 else 1       # 1 .. 4 candidates; DCT2 alone on a side of 64
        return [(th, tv, 22 + 5 * k + p % 7, (p + k) & 1) for k, (th, tv) in enumerate(cands[:n])]

    shapes = [(4, 4, 0, 8, [0, 1, 2], [(15, 1)]), (8, 4, 1, 10, [1, 18, 34, 66], []), (4, 16, 2, 12, [2, 50], []), (8, 8, 0, 10, [0, 34], [(0, 0), (7, 1)]),
              (16, 16, 2, 8, [1, 66, 50], []), (32, 8, 0, 12, [3, 0], [(5, 0)]), (64, 16, 1, 10, [18, 60], []), (64, 64, 0, 10, [0], [(5, 1), (0, 0)])]
    lv = icu.make_level(rng, shapes, tus_of)
    assert lv.n_intra == 19 and lv.n_mip == 6 and {lv.blk_arr[i].multiRefIdx for i in range(8)} == {0, 1, 2}
    per_pred = np.bincount([lv.tu_arr[k].pred for k in range(lv.n_tu)], minlength=25)
    assert set(per_pred) == {1, 2, 3, 4}
    assert {(lv.tu_arr[k].typeHor, lv.tu_arr[k].typeVer) for k in range(lv.n_tu)} == set(cands)
    assert _same(lv) == (64, 64, 0)
    # the same table with its TU jobs shuffled: out[k] follows tuJobs[k]
    order = rng.permutation(lv.n_tu)
    s = icu.Level(lv.blocks, lv.plane, lv.tus, order=order)
    _same(s)
    got, ref = _call(s)[0], _call(lv)[0]
    assert [icu.tu_fields(got[k]) | {"outOff": 0} for k in range(s.n_tu)] == [icu.tu_fields(ref[int(o)]) | {"outOff": 0} for o in order]


def test_uniform_both_ways_and_empty_tables():
    rng = np.random.default_rng(42)
    shapes = [(8, 8, m, 10, [1, 18, 50], [(3, 1)] if m == 0 else []) for m in (0, 1, 2, 0)]
    real = lambda p, b: [(lib.DCT2, lib.DCT2, 30, 0), (lib.DST7, lib.DCT8, 30, 1)]       # noqa: E731
    lv = icu.make_level(rng, shapes, real)
    assert _same(lv) == (8, 8, 1)
    with_ts = icu.Level(lv.blocks, lv.plane, lv.tus + [(2, lib.TRSKIP, lib.TRSKIP, 30, 0)])
    assert _same(with_ts) == (8, 8, 0)
    two_sizes = icu.make_level(rng, shapes + [(8, 4, 0, 10, [1], [])], real)
    assert _same(two_sizes) == (8, 8, 0)
    # the prediction + residual pass alone; one table empty; everything empty
    assert _same(icu.Level(lv.blocks, lv.plane, [])) == (0, 0, 0)
    for b in lv.blocks:
        b["mip"] = []
    no_mip = icu.Level(lv.blocks, lv.plane, [(p, lib.DCT2, lib.DCT2, 30, 0) for p in range(12)])
    assert no_mip.n_mip == 0 and _same(no_mip) == (8, 8, 1)
    for b in lv.blocks:
        b["modes"], b["mip"] = [], [(1, 0)] if b["m"] == 0 else []
    no_intra = icu.Level(lv.blocks, lv.plane, [(p, lib.DCT2, lib.DCT2, 30, 0) for p in range(2)])
    assert no_intra.n_intra == 0 and no_intra.n_mip == 2 and _same(no_intra) == (8, 8, 1)
    L = lib.load()
    assert L.vtmhip_intra_chain_make_tu_jobs(None, 0, None, 0, None, 0, None, 0, None, None, None, None) == lib.OK


def test_the_base_table_of_the_rejections_is_well_formed():
    lv = icu.base_level()
    assert (lv.n_intra, lv.n_mip, lv.n_tu) == (6, 3, 12)
    assert _same(lv) == (64, 16, 0)


@pytest.mark.parametrize("name,defect", icu.DEFECTS, ids=[n for n, _ in icu.DEFECTS])
def test_a_malformed_table_is_rejected_whole(name, defect):
    L = lib.load()
    lv = icu.base_level()
    defect(lv)
    out = np.full(lv.n_tu * C.sizeof(TuJob), icu.FILL, np.uint8)
    mw, mh, uni = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    st = L.vtmhip_intra_chain_make_tu_jobs(C.addressof(lv.blk_arr), len(lv.blocks), C.addressof(lv.intra_arr), lv.n_intra, C.addressof(lv.mip_arr), lv.n_mip,
                                           C.addressof(lv.tu_arr), lv.n_tu, out.ctypes.data, C.byref(mw), C.byref(mh), C.byref(uni))
    assert st == lib.E_INVALID
    assert (out == icu.FILL).all() and (mw.value, mh.value, uni.value) == (-7, -7, -7)


def test_null_pointers_and_negative_counts():
    L = lib.load()
    lv = icu.base_level()
    good = [C.addressof(lv.blk_arr), len(lv.blocks), C.addressof(lv.intra_arr), lv.n_intra, C.addressof(lv.mip_arr), lv.n_mip, C.addressof(lv.tu_arr), lv.n_tu]
    out = (TuJob * lv.n_tu)()
    assert L.vtmhip_intra_chain_make_tu_jobs(*good, C.addressof(out), None, None, None) == lib.OK
    for k in range(8):
        bad = list(good)
        bad[k] = -1 if k & 1 else None
        assert L.vtmhip_intra_chain_make_tu_jobs(*bad, C.addressof(out), None, None, None) == lib.E_INVALID, k
    assert L.vtmhip_intra_chain_make_tu_jobs(*good, None, None, None, None) == lib.E_INVALID
    with pytest.raises(VtmHipError):
        lv.tu_arr[0].pred = 99
        _call(lv)
