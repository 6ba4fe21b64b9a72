"""CPU: the tables of the intra chroma residual chain.  Struct layouts, the pins that must not move, vtmhip_intra_chroma_chain_make_jobs (the host form of the
entry's checks and expansion) against a Python restatement on a mixed table, and every rejection -- one table per defect."""
import ctypes as C

import numpy as np
import pytest

import cclm_util as cu
import intra_chroma_chain_util as ccu
from vtm_amd import lib
from vtm_amd.device import intra_chroma_chain_make_jobs
from vtm_amd.lib import (IntraChromaBlock, IntraChromaJob, IntraChromaJointJob, IntraChromaJointResult, IntraChromaTuJob, IntraTuResult, JccrJob, TuJob,
                         VtmHipError)


def test_struct_sizes_and_the_pins_that_must_not_move():
    L = lib.load()
    assert (C.sizeof(IntraChromaTuJob), C.sizeof(IntraChromaJointJob), C.sizeof(IntraChromaJointResult)) == (24, 24, 48)
    assert [L.vtmhip_intra_chroma_chain_struct_size(k) for k in (0, 1, 2, 3, -1)] == [24, 24, 48, -1, -1]
    assert IntraChromaTuJob.chromaAdj.offset == 20 and IntraChromaJointJob.chromaAdj.offset == 20 and IntraChromaJointResult.fwdDist.offset == 32
    assert L.vtmhip_abi_version() == 6 and L.vtmhip_struct_size(36) == -1
    assert L.vtmhip_intra_chroma_struct_size(3) == -1 and L.vtmhip_intra_chain_struct_size(2) == -1 and L.vtmhip_jccr_struct_size(3) == -1
    assert (C.sizeof(IntraChromaBlock), C.sizeof(IntraChromaJob), C.sizeof(TuJob), C.sizeof(JccrJob), C.sizeof(IntraTuResult)) == (64, 24, 40, 48, 24)


def _call(lv):
    return intra_chroma_chain_make_jobs(lv.blk_arr if lv.blocks else None, lv.job_arr if lv.n_pred else None, lv.tu_arr if lv.n_tu else None,
                                        lv.joint_arr if lv.n_joint else None)


def _same(lv):
    tu, jt, pt, pj, crs = _call(lv)
    etu, ejt, ept, epj, ecrs = ccu.expand(*lv.tables())
    assert len(tu) == lv.n_tu and [ccu.tu_fields(j) for j in tu] == etu
    assert len(jt) == lv.n_joint and [ccu.jccr_fields(j) for j in jt] == ejt
    assert (pt, pj, crs) == (ept, epj, ecrs)
    return pt, pj, crs


def _mixed_cands(p, b):
    """1 .. 4 single jobs and 0 .. 6 joint jobs per prediction"""
    single = [(0, 0), (1, 0), (0, 1), (1, 1)][:1 + p % 4]
    joint = [(m, ts) for ts in (0, 1) for m in (1, 2, 3)][:p % 7]
    adj = ccu.ADJS[p % 5]
    return ([(c, ts, 22 + 5 * k + p % 7, (p + k) & 1, adj) for k, (c, ts) in enumerate(single)],
            [(m, (p + k) & 1, ts, 25 + 3 * k, k & 1, adj) for k, (m, ts) in enumerate(joint)])


def test_expansion_of_a_mixed_table():
    rng = np.random.default_rng(41)
    shapes = [(w, h, (8, 10, 12)[(i + j) % 3], "random", cu.AVAIL_CLASSES[(2 * i + j) % 6], bool(i & 1), bool(j & 1), [(0, 1, 18, 50)[(i + j) % 4], 67 + (i + 2 * j) % 3])
              for i, w in enumerate(cu.SIDES) for j, h in enumerate(cu.SIDES)]
    lv = ccu.make_level(rng, shapes, _mixed_cands)
    assert len(lv.blocks) == 16 and lv.n_pred == 32 and {lv.job_arr[k].mode >= cu.LM for k in range(32)} == {False, True}
    assert set(np.bincount([t.pred for t in lv.tables()[2]], minlength=32)) == {1, 2, 3, 4}
    assert set(np.bincount([t.pred for t in lv.tables()[3]], minlength=32)) == {0, 1, 2, 3, 4, 5, 6}
    assert {t.component for t in lv.tables()[2]} == {0, 1} and {(t.cbfMask, t.signFlag) for t in lv.tables()[3]} == {(m, s) for m in (1, 2, 3) for s in (0, 1)}
    assert {t.chromaAdj for t in lv.tables()[2]} == set(ccu.ADJS)
    assert _same(lv) == ((32, 32, 0), (32, 32, 0), 1)
    # the same tables shuffled -- the prediction jobs too: out[k] follows its own table
    order = (rng.permutation(lv.n_tu), rng.permutation(lv.n_joint))
    s = ccu.Level(lv.blocks, lv.plane, lv.singles, lv.joints, order=order)
    _same(s)
    got, ref = _call(s), _call(lv)
    assert [ccu.tu_fields(got[0][k]) | {"outOff": 0} for k in range(s.n_tu)] == [ccu.tu_fields(ref[0][int(o)]) | {"outOff": 0} for o in order[0]]
    assert [ccu.jccr_fields(got[1][k]) | {"outOff": 0} for k in range(s.n_joint)] == [ccu.jccr_fields(ref[1][int(o)]) | {"outOff": 0} for o in order[1]]
    _same(ccu.make_level(np.random.default_rng(41), shapes, _mixed_cands, job_order=np.random.default_rng(3).permutation(32)))


def test_uniform_and_crs_both_ways_and_empty_tables():
    rng = np.random.default_rng(42)
    shapes = [(8, 8, 10, "random", "full", False, False, [1, 18, 67]) for _ in range(3)]
    plain = lambda p, b: ([(0, 0, 30, 0, 0), (1, 0, 30, 1, 0)], [(1 + p % 3, 0, 0, 30, 0, 0)])       # noqa: E731
    lv = ccu.make_level(rng, shapes, plain)
    assert _same(lv) == ((8, 8, 1), (8, 8, 1), 0)
    # transform skip alone makes a table non-uniform: one table at a time
    assert _same(ccu.Level(lv.blocks, lv.plane, lv.singles + [(2, 1, 1, 30, 0, 0)], lv.joints)) == ((8, 8, 0), (8, 8, 1), 0)
    assert _same(ccu.Level(lv.blocks, lv.plane, lv.singles, lv.joints + [(2, 3, 1, 1, 30, 0, 0)])) == ((8, 8, 1), (8, 8, 0), 0)
    # one adj in either table switches the CRS instantiations on
    assert _same(ccu.Level(lv.blocks, lv.plane, lv.singles + [(0, 1, 0, 30, 0, 2048)], lv.joints)) == ((8, 8, 1), (8, 8, 1), 1)
    assert _same(ccu.Level(lv.blocks, lv.plane, lv.singles, lv.joints + [(0, 2, 1, 0, 30, 0, 1)])) == ((8, 8, 1), (8, 8, 1), 1)
    # a second size, in the single table only
    blocks, plane = ccu.make_blocks(rng, shapes + [(8, 4, 10, "random", "both", False, False, [1])])
    assert _same(ccu.Level(blocks, plane, lv.singles + [(9, 0, 0, 30, 0, 0)], lv.joints)) == ((8, 8, 0), (8, 8, 1), 0)
    # one table empty; the prediction + residual pass alone; nothing at all
    assert _same(ccu.Level(lv.blocks, lv.plane, lv.singles, [])) == ((8, 8, 1), (0, 0, 0), 0)
    assert _same(ccu.Level(lv.blocks, lv.plane, [], lv.joints)) == ((0, 0, 0), (8, 8, 1), 0)
    assert _same(ccu.Level(lv.blocks, lv.plane, [], [])) == ((0, 0, 0), (0, 0, 0), 0)
    L = lib.load()
    assert L.vtmhip_intra_chroma_chain_make_jobs(None, 0, None, 0, None, 0, None, 0, None, None, None, None, None, None, None) == lib.OK


def test_the_base_table_of_the_rejections_is_well_formed():
    lv = ccu.base_level()
    assert (len(lv.blocks), lv.n_pred, lv.n_tu, lv.n_joint) == (3, 7, 14, 14)
    assert _same(lv) == ((32, 16, 0), (32, 16, 0), 1)


def _raw_call(L, lv, out_tu, out_joint, *plan):
    return L.vtmhip_intra_chroma_chain_make_jobs(C.addressof(lv.blk_arr), len(lv.blocks), C.addressof(lv.job_arr), lv.n_pred, C.addressof(lv.tu_arr), lv.n_tu,
                                                 C.addressof(lv.joint_arr), lv.n_joint, out_tu, out_joint, *plan)


@pytest.mark.parametrize("name,defect", ccu.DEFECTS, ids=[n for n, _ in ccu.DEFECTS])
def test_a_malformed_table_is_rejected_whole(name, defect):
    L = lib.load()
    lv = ccu.base_level()
    defect(lv)
    out_tu, out_joint = np.full(lv.n_tu * C.sizeof(TuJob), ccu.FILL, np.uint8), np.full(lv.n_joint * C.sizeof(JccrJob), ccu.FILL, np.uint8)
    mw, mh, ut, uj, crs = (C.c_int * 2)(-7, -7), (C.c_int * 2)(-7, -7), C.c_int(-7), C.c_int(-7), C.c_int(-7)
    assert _raw_call(L, lv, out_tu.ctypes.data, out_joint.ctypes.data, mw, mh, C.byref(ut), C.byref(uj), C.byref(crs)) == lib.E_INVALID
    assert (out_tu == ccu.FILL).all() and (out_joint == ccu.FILL).all()
    assert (list(mw), list(mh), ut.value, uj.value, crs.value) == ([-7, -7], [-7, -7], -7, -7, -7)


def test_null_pointers_and_negative_counts():
    L = lib.load()
    lv = ccu.base_level()
    good = [C.addressof(lv.blk_arr), len(lv.blocks), C.addressof(lv.job_arr), lv.n_pred, C.addressof(lv.tu_arr), lv.n_tu, C.addressof(lv.joint_arr), lv.n_joint]
    out_tu, out_joint = (TuJob * lv.n_tu)(), (JccrJob * lv.n_joint)()
    none5 = [None] * 5
    assert L.vtmhip_intra_chroma_chain_make_jobs(*good, C.addressof(out_tu), C.addressof(out_joint), *none5) == lib.OK
    for k in range(8):
        bad = list(good)
        bad[k] = -1 if k & 1 else None
        assert L.vtmhip_intra_chroma_chain_make_jobs(*bad, C.addressof(out_tu), C.addressof(out_joint), *none5) == lib.E_INVALID, k
    assert L.vtmhip_intra_chroma_chain_make_jobs(*good, None, C.addressof(out_joint), *none5) == lib.E_INVALID
    assert L.vtmhip_intra_chroma_chain_make_jobs(*good, C.addressof(out_tu), None, *none5) == lib.E_INVALID
    with pytest.raises(VtmHipError):
        lv.tu_arr[0].pred = 99
        _call(lv)
