"""GPU parity at the decision edges of bdof_kernel / dmvr_kernel / dmvr_chroma_kernel: the constructed tables of bipred_edge_util (early termination and
BDOF switch-off at their thresholds, ties, the +-8 branches, zero denominators, the centre's discount, vectors beyond clipMv, saturated and unsaturated BDOF
refinements, both output clips) at 8, 10 and 12 bits, bit-exact against the oracle -- which test_bipred_edges.py pins to the reference on the same tables.
Every test asserts the census of its table BEFORE it asks the device: an expectation that no longer reaches the edges fails here, not silently."""
import numpy as np
import pytest

import bipred_edge_util as U
import oracle_lib as ol
import test_bipred_edges as cpu
from vtm_amd.lib import DmvrJob, PicParams, PredJob

pytestmark = pytest.mark.gpu
W, H = U.PIC_W, U.PIC_H
MVD_ROOM = 64 * 2      # every buffer of vector differences has room for 64-region rows, whatever the call's row is: a wrong stride then shows as wrong values


def _dmvr_jobs(tab, select=None, ref_shift=0):
    """(DmvrJob table, job indices, expected prediction, expected epilogue output, samples) for the luma plane."""
    ks = list(range(tab.n)) if select is None else select
    jobs, exp, pos = (DmvrJob * len(ks))(), tab.expect(), 0
    pred, out = [], []
    for i, k in enumerate(ks):
        t, j = tab.jobs[k], jobs[i]
        w, h = t["w"], t["h"]
        for l in range(2):
            j.refOff[l], j.refStride[l] = ref_shift + t["off"][l], t["S"]
        j.mv[0][0], j.mv[0][1], j.mv[1][0], j.mv[1][1] = t["mv"]
        j.orgOff, j.orgStride, j.puX, j.puY = t["y"] * W + t["x"], W, t["x"], t["y"]
        j.predOff = j.outOff = pos
        j.predStride = j.outStride = w
        j.width, j.height, j.bitDepth, j.bioApplied, j.epilogue = w, h, tab.bd, t["bio"], 1 + k % 2
        o = tab.org[t["y"]:t["y"] + h, t["x"]:t["x"] + w].astype(np.int32)
        pred.append(exp["pred"][k].reshape(-1))
        out.append(((o if j.epilogue == 1 else 2 * o) - exp["pred"][k]).astype(np.int16).reshape(-1))
        pos += w * h
    return jobs, ks, np.concatenate(pred), np.concatenate(out), pos


def _check_mvd(tab, ks, got, regions):
    exp = tab.expect()["mvd"]
    got = got[:len(ks) * regions * 2].reshape(len(ks), regions, 2)
    for i, k in enumerate(ks):
        ns = tab.jobs[k]["nsub"]
        assert np.array_equal(got[i, :ns], exp[k, :ns]), (tab.name, tab.bd, k, tab.jobs[k]["label"], got[i, :ns], exp[k, :ns])


@pytest.mark.parametrize("bd", U.DEPTHS)
@pytest.mark.parametrize("name", U.DMVR_TABLES)
def test_dmvr_edges_match_oracle(ctx, name, bd):
    """vtmhip_dmvr_batch_dev: prediction, both epilogues and the vector differences.  maxWidth = maxHeight = 32: four regions per row of the vector
    differences (the 32 x 32 PU fills all four with different values); the tie table also goes through a 128 x 128 launch (64 regions)."""
    cpu.test_dmvr_census(name, bd)
    tab = U.dmvr_table(name, bd)
    jobs, ks, pred, out, pos = _dmvr_jobs(tab)
    pic = PicParams(W, H, U.CTU, bd, 0)
    d_ref, d_org, d_jobs = ctx.to_device(tab.refs), ctx.to_device(tab.org.reshape(-1)), ctx.to_device(np.frombuffer(jobs, np.uint8))
    for mx in ((32, 128) if name == "tie" else (32,)):
        regions = (mx // 16) ** 2
        d_pred, d_out, d_mvd = ctx.to_device(np.full(pos, -1, np.int16)), ctx.to_device(np.full(pos, -1, np.int16)), ctx.to_device(np.full(tab.n * MVD_ROOM, 99, np.int32))
        ctx.dmvr_batch(pic, d_org.ptr, d_ref.ptr, d_pred.ptr, d_out.ptr, d_jobs.ptr, tab.n, mx, mx, d_mvd.ptr)
        _check_mvd(tab, ks, d_mvd.to_host(np.int32), regions)
        got = d_pred.to_host(np.int16)
        if not np.array_equal(got, pred):
            at = 0
            for k in ks:      # name the first job that differs
                n = tab.jobs[k]["w"] * tab.jobs[k]["h"]
                assert np.array_equal(got[at:at + n], pred[at:at + n]), (name, bd, mx, k, tab.jobs[k]["label"], tab.jobs[k]["bio"])
                at += n
        assert np.array_equal(d_out.to_host(np.int16), out), (name, bd, mx)


@pytest.mark.parametrize("bd", U.DEPTHS)
@pytest.mark.parametrize("name", U.DMVR_TABLES)
def test_dmvr_chroma_edges_match_oracle(ctx, name, bd):
    """vtmhip_dmvr_chroma_batch_dev on the vector differences of the tables, both chroma planes: unmoved sub-PUs and moves by +-8, 24, +-32 and the
    division results, vectors on the clipMv bounds; the row stride of the vector differences is 4 regions."""
    cpu.test_dmvr_tables_move_chroma_every_way(bd)
    tab = U.dmvr_table(name, bd)
    exp = tab.expect()
    pic = PicParams(W, H, U.CTU, bd, 0)
    d_ref, d_mvd = ctx.to_device(tab.crefs), ctx.to_device(np.concatenate([exp["mvd"].reshape(-1), np.full(tab.n * MVD_ROOM - exp["mvd"].size, 99, np.int32)]))
    for c in range(2):
        jobs, pos, pred, out = (DmvrJob * tab.n)(), 0, [], []
        for k, t in enumerate(tab.jobs):
            j, w, h = jobs[k], t["w"], t["h"]
            for l in range(2):
                j.refOff[l], j.refStride[l] = t["offc"][c][l], t["Sc"]
            j.mv[0][0], j.mv[0][1], j.mv[1][0], j.mv[1][1] = t["mv"]
            j.orgOff, j.orgStride, j.puX, j.puY, j.mvdRow = (t["y"] // 2) * (W // 2) + t["x"] // 2, W // 2, t["x"], t["y"], k
            j.predOff = j.outOff = pos
            j.predStride = j.outStride = w // 2
            j.width, j.height, j.bitDepth, j.epilogue = w, h, bd, 1 + (k // 2) % 2
            o = tab.orgc[c][t["y"] // 2:(t["y"] + h) // 2, t["x"] // 2:(t["x"] + w) // 2].astype(np.int32)
            e = exp["cpred"][k][c]
            pred.append(e.reshape(-1))
            out.append(((o if j.epilogue == 1 else 2 * o) - e).astype(np.int16).reshape(-1))
            pos += w * h // 4
        d_org, d_jobs = ctx.to_device(tab.orgc[c].reshape(-1)), ctx.to_device(np.frombuffer(jobs, np.uint8))
        d_pred, d_out = ctx.to_device(np.full(pos, -1, np.int16)), ctx.to_device(np.full(pos, -1, np.int16))
        ctx.dmvr_chroma_batch(pic, d_org.ptr, d_ref.ptr, d_pred.ptr, d_out.ptr, d_jobs.ptr, tab.n, 32, 32, d_mvd.ptr)
        got, want, at = d_pred.to_host(np.int16), np.concatenate(pred), 0
        for k, t in enumerate(tab.jobs):
            n = t["w"] * t["h"] // 4
            assert np.array_equal(got[at:at + n], want[at:at + n]), (name, bd, c, k, t["label"], exp["mvd"][k, :t["nsub"]])
            at += n
        assert np.array_equal(d_out.to_host(np.int16), np.concatenate(out)), (name, bd, c)


def _bdof_jobs(tab, select=None, ref_shift=0):
    ks = list(range(tab.n)) if select is None else select
    jobs, exp, pos, pred, out = (PredJob * len(ks))(), tab.expect(), 0, [], []
    for i, k in enumerate(ks):
        t, j = tab.jobs[k], jobs[i]
        w, h = t["w"], t["h"]
        for l in range(2):
            j.refOff[l], j.refStride[l] = ref_shift + t["off"][l], t["S"]
        j.mv[0][0], j.mv[0][1], j.mv[1][0], j.mv[1][1] = t["mv"]
        j.orgOff, j.orgStride = t["y"] * W + t["x"], W
        j.predOff = j.outOff = pos
        j.predStride = j.outStride = w
        j.width, j.height, j.mode, j.bitDepth, j.epilogue = w, h, 2, tab.bd, 1 + k % 2
        o = tab.org[t["y"]:t["y"] + h, t["x"]:t["x"] + w].astype(np.int32)
        pred.append(exp["pred"][k].reshape(-1))
        out.append(((o if j.epilogue == 1 else 2 * o) - exp["pred"][k]).astype(np.int16).reshape(-1))
        pos += w * h
    return jobs, ks, np.concatenate(pred), np.concatenate(out), pos


@pytest.mark.parametrize("bd", U.DEPTHS)
def test_bdof_edges_match_oracle(ctx, bd):
    """vtmhip_bdof_batch_dev: prediction + both epilogues, and a prediction-only call."""
    cpu.test_bdof_census(bd)
    tab = U.bdof_table(bd)
    jobs, ks, pred, out, pos = _bdof_jobs(tab)
    d_ref, d_org, d_jobs = ctx.to_device(tab.refs), ctx.to_device(tab.org.reshape(-1)), ctx.to_device(np.frombuffer(jobs, np.uint8))
    d_pred, d_out = ctx.to_device(np.full(pos, -1, np.int16)), ctx.to_device(np.full(pos, -1, np.int16))
    ctx.bdof_batch(d_org.ptr, d_ref.ptr, d_pred.ptr, d_out.ptr, d_jobs.ptr, tab.n, 32, 32)
    got, at = d_pred.to_host(np.int16), 0
    for k in ks:
        n = tab.jobs[k]["w"] * tab.jobs[k]["h"]
        assert np.array_equal(got[at:at + n], pred[at:at + n]), (bd, k, tab.jobs[k]["group"], tab.jobs[k]["mv"])
        at += n
    assert np.array_equal(d_out.to_host(np.int16), out), bd
    d_pred2 = ctx.to_device(np.full(pos, -1, np.int16))
    ctx.bdof_batch(0, d_ref.ptr, d_pred2.ptr, 0, d_jobs.ptr, tab.n, 32, 32)
    assert np.array_equal(d_pred2.to_host(np.int16), pred), bd


def test_merge_candidates_at_the_edges(ctx, bd=10):
    """vtmhip_merge_cand_satd_batch_dev launches the same bdof_kernel / dmvr_kernel (only its distortion stage has a `uniform` form), so once is enough: the
    16 x 16 jobs of the threshold and tie tables as its DMVR list, the 16 x 16 stripe jobs as its BDOF list, both distortion forms."""
    cpu.test_dmvr_census("thr", bd), cpu.test_dmvr_census("tie", bd), cpu.test_bdof_census(bd)
    thr, tie, bdo = U.dmvr_table("thr", bd), U.dmvr_table("tie", bd), U.bdof_table(bd)
    org = tie.org
    parts, preds, tabs, shift = [], [], [], 0
    for tab, pick in ((thr, lambda t: True), (tie, lambda t: True), (bdo, lambda t: t["group"] in ("diag", "anti"))):
        ks = [k for k, t in enumerate(tab.jobs) if (t["w"], t["h"]) == (16, 16) and pick(t)]
        tabs.append((tab, ks, shift))
        shift += tab.refs.size
    dj = [_dmvr_jobs(t, ks, s) for t, ks, s in tabs[:2]]
    bj = _bdof_jobs(*tabs[2])
    n_d, n_b = len(dj[0][1]) + len(dj[1][1]), len(bj[1])
    assert n_d >= 100 and n_b >= 20
    dmvr, bdof = (DmvrJob * n_d)(), bj[0]
    for i in range(n_d):
        src = dj[0][0][i] if i < len(dj[0][1]) else dj[1][0][i - len(dj[0][1])]
        np.frombuffer(dmvr, np.uint8).reshape(n_d, -1)[i] = np.frombuffer(src, np.uint8)
    pos = 0
    for tab_jobs in (bdof, dmvr):      # the order of the distortion list: plain, BDOF, DMVR
        for j in tab_jobs:
            j.predOff, j.epilogue = pos, 0
            pos += 256
    want_pred = np.concatenate([bj[2], dj[0][2], dj[1][2]])
    dist = []
    for (tab, ks, _s) in (tabs[2], tabs[0], tabs[1]):
        for k in ks:
            t = tab.jobs[k]
            dist.append(ol.o_dist(1, np.ascontiguousarray(org[t["y"]:t["y"] + 16, t["x"]:t["x"] + 16]), np.ascontiguousarray(tab.expect()["pred"][k]), 16, 16))
    d_ref = ctx.to_device(np.concatenate([thr.refs, tie.refs, bdo.refs]))
    d_org = ctx.to_device(org.reshape(-1))
    d_b, d_d = ctx.to_device(np.frombuffer(bdof, np.uint8)), ctx.to_device(np.frombuffer(dmvr, np.uint8))
    pic = PicParams(W, H, U.CTU, bd, 0)
    for uniform in (False, True):
        d_pred, d_dist, d_mvd = ctx.to_device(np.full(pos, -1, np.int16)), ctx.alloc(8 * (n_b + n_d)), ctx.to_device(np.full(n_d * MVD_ROOM, 99, np.int32))
        ctx.merge_cand_satd_batch(pic, d_org.ptr, d_ref.ptr, d_pred.ptr, 0, 0, d_b.ptr, n_b, d_d.ptr, n_d, d_mvd.ptr, 16, 16, d_dist.ptr, uniform=uniform)
        assert np.array_equal(d_pred.to_host(np.int16), want_pred), uniform
        assert d_dist.to_host(np.uint64).tolist() == dist, uniform
        mv = d_mvd.to_host(np.int32)[:2 * n_d].reshape(n_d, 2)
        assert np.array_equal(mv[:len(dj[0][1])], thr.expect()["mvd"][dj[0][1], 0]) and np.array_equal(mv[len(dj[0][1]):], tie.expect()["mvd"][dj[1][1], 0]), uniform
