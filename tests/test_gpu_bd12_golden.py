"""GPU replay of tests/golden/bd12.npz: 12-bit outputs recorded from the real reference (DMVR, BDOF, motion compensation, xT / xIT, quant /
dequant; generator tests/golden/gen_bd12_golden.py).  It catches a mistake that the oracle and a kernel share, and it runs where the reference library
is not built."""
import ctypes as C
import os

import numpy as np
import pytest

from vtm_amd.lib import DmvrJob, PicParams, PredJob, QuantJob, TrJob

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MTS_TYPES = {0: (0, 0), 2: (2, 2), 3: (1, 2), 4: (2, 1), 5: (1, 1)}


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(G, "bd12.npz"))


@pytest.fixture(scope="module")
def pictures(z):
    import sys
    sys.path.insert(0, G)
    import gen_bd12_golden as gen
    P, org = gen.planes()
    assert [int(P[l][c][0].astype(np.int64).sum()) for l in range(2) for c in range(3)] == z["plane_sums"].tolist()
    return gen, P, org


def _refs(P, comps):
    """One device buffer holding the padded planes [l][c] for c in comps, and the base offset of each."""
    bufs, base, at = [], {}, 0
    for l in range(2):
        for c in comps:
            base[(l, c)] = at
            bufs.append(P[l][c][0].reshape(-1))
            at += P[l][c][0].size
    return np.concatenate(bufs), base


def test_dmvr_bd12_matches_reference_golden(ctx, z, pictures):
    gen, P, org = pictures
    rows = z["dmvr"]
    n = len(rows)
    refs, base = _refs(P, (0,))
    jobs = (DmvrJob * n)()
    pos, offs = 0, []
    for k, (x, y, w, h, m0h, m0v, m1h, m1v, bio) in enumerate(rows.tolist()):
        j = jobs[k]
        for l in range(2):
            j.refOff[l], j.refStride[l] = base[(l, 0)] + P[l][0][1] + y * P[l][0][2] + x, P[l][0][2]
        j.mv[0][0], j.mv[0][1], j.mv[1][0], j.mv[1][1] = m0h, m0v, m1h, m1v
        j.orgOff, j.orgStride, j.puX, j.puY = y * gen.W + x, gen.W, x, y
        j.predOff, j.predStride, j.outOff, j.outStride = pos, w, pos, w
        j.width, j.height, j.bitDepth, j.bioApplied, j.epilogue = w, h, 12, bio, 0
        offs.append(pos)
        pos += w * h
    d_ref, d_org = ctx.to_device(refs), ctx.to_device(org.reshape(-1))
    d_jobs = ctx.to_device(np.frombuffer(jobs, np.uint8))
    regions = 4   # 16 x 16 regions of the 32 x 32 bound: the vector differences of job k start at row k * regions
    d_pred, d_mvd = ctx.alloc(2 * pos), ctx.alloc(4 * n * regions * 2)
    ctx.dmvr_batch(PicParams(gen.W, gen.H, 128, 12, 0), d_org.ptr, d_ref.ptr, d_pred.ptr, 0, d_jobs.ptr, n, 32, 32, d_mvd.ptr)
    assert np.array_equal(d_pred.to_host(np.int16), z["dmvr_pred"])
    got = d_mvd.to_host(np.int32).reshape(n, regions * 2)
    at = 0
    for k, (x, y, w, h, *_r) in enumerate(rows.tolist()):
        nsub = (w // min(w, 16)) * (h // min(h, 16))
        assert np.array_equal(got[k, :2 * nsub], z["dmvr_mvd"][at:at + 2 * nsub]), k
        at += 2 * nsub


def test_bdof_bd12_matches_reference_golden(ctx, z, pictures):
    gen, P, org = pictures
    rows = z["bdof"]
    n = len(rows)
    refs, base = _refs(P, (0,))
    jobs = (PredJob * n)()
    pos = 0
    for k, (x, y, w, h, *mv) in enumerate(rows.tolist()):
        j = jobs[k]
        for l in range(2):
            j.refOff[l], j.refStride[l] = base[(l, 0)] + P[l][0][1] + y * P[l][0][2] + x, P[l][0][2]
        j.mv[0][0], j.mv[0][1], j.mv[1][0], j.mv[1][1] = mv
        j.predOff, j.predStride = pos, w
        j.width, j.height, j.mode, j.bitDepth, j.epilogue = w, h, 2, 12, 0
        pos += w * h
    d_ref, d_jobs, d_pred = ctx.to_device(refs), ctx.to_device(np.frombuffer(jobs, np.uint8)), ctx.alloc(2 * pos)
    ctx.bdof_batch(0, d_ref.ptr, d_pred.ptr, 0, d_jobs.ptr, n, 32, 32)
    assert np.array_equal(d_pred.to_host(np.int16), z["bdof_pred"])


def test_motion_compensation_bd12_matches_reference_golden(ctx, z, pictures):
    gen, P, org = pictures
    rows = z["mc"]
    n = len(rows)
    refs, base = _refs(P, (0, 1, 2))
    jobs = (PredJob * n)()
    pos = 0
    for k, (comp, x, y, w, h, mode, m0h, m0v, m1h, m1v, alt) in enumerate(rows.tolist()):
        cx, cy = (x // 2, y // 2) if comp else (x, y)
        j = jobs[k]
        for l in range(2):
            j.refOff[l], j.refStride[l] = base[(l, comp)] + P[l][comp][1] + cy * P[l][comp][2] + cx, P[l][comp][2]
        j.mv[0][0], j.mv[0][1], j.mv[1][0], j.mv[1][1] = m0h, m0v, m1h, m1v
        j.predOff, j.predStride, j.outOff, j.outStride = pos, w, pos, w
        j.width, j.height, j.mode, j.epilogue, j.bitDepth, j.useAltHpelIf, j.chroma = w, h, mode, 0, 12, alt, int(comp != 0)
        pos += w * h
    d_ref, d_org = ctx.to_device(refs), ctx.to_device(org.reshape(-1))
    d_jobs, d_pred = ctx.to_device(np.frombuffer(jobs, np.uint8)), ctx.alloc(2 * pos)
    ctx.motion_compensation_batch(d_org.ptr, d_ref.ptr, d_pred.ptr, None, d_jobs.ptr, n, 32, 32)
    assert np.array_equal(d_pred.to_host(np.int16), z["mc_pred"])
    assert z["mc_pred"].min() == 0 and z["mc_pred"].max() == 4095


def test_transforms_bd12_match_reference_golden(ctx, z):
    rows = z["tr"]
    n = len(rows)
    jobs = (TrJob * n)()
    at = 0
    for k, (w, h, mts) in enumerate(rows.tolist()):
        j = jobs[k]
        j.srcOff = j.dstOff = at
        j.srcStride = j.dstStride = w
        j.width, j.height, j.bitDepth = w, h, 12
        j.typeHor, j.typeVer = MTS_TYPES[mts]
        at += w * h
    d_jobs = ctx.to_device(np.frombuffer(jobs, np.uint8))
    d_coef = ctx.alloc(4 * at, np.int32)
    ctx.xT_batch(ctx.to_device(z["tr_resi"]).ptr, d_coef.ptr, d_jobs.ptr, n, 64, 64, None)
    assert np.array_equal(d_coef.to_host(np.int32), z["tr_coef"])
    # the inverse of the (int16-clipped, zeroed-out) coefficients the generator fed xIT
    coef = np.clip(z["tr_coef"], -32768, 32767).astype(np.int32)
    at = 0
    for (w, h, mts) in rows.tolist():
        th, tv = MTS_TYPES[mts]
        c2 = coef[at:at + w * h].reshape(h, w)
        zw = 16 if (th != 0 and w == 32) else max(0, w - 32)
        zh = 16 if (tv != 0 and h == 32) else max(0, h - 32)
        if zw:
            c2[:, w - zw:] = 0
        if zh:
            c2[h - zh:, :] = 0
        at += w * h
    d_back = ctx.alloc(2 * at, np.int16)
    ctx.xIT_batch(ctx.to_device(coef).ptr, d_back.ptr, d_jobs.ptr, n, 64, 64)
    assert np.array_equal(d_back.to_host(np.int16), z["tr_back"])


def test_quant_dequant_bd12_match_reference_golden(ctx, z):
    rows = z["quant"]
    n = len(rows)
    jobs = (QuantJob * n)()
    at = 0
    for k, (w, h, qp, irap, ts, _s) in enumerate(rows.tolist()):
        j = jobs[k]
        bq = max(qp + 24, 4) if ts else qp + 24   # QpParam: the transform-skip QP' is at least 4
        j.srcOff, j.dstOff, j.width, j.height, j.qpPer, j.qpRem = at, at, w, h, bq // 6, bq % 6
        j.bitDepth, j.isIRAP, j.isTransformSkip = 12, irap, ts
        at += w * h
    d_jobs = ctx.to_device(np.frombuffer(jobs, np.uint8))
    d_q, d_du, d_dq = ctx.alloc(4 * at, np.int32), ctx.alloc(4 * at, np.int32), ctx.alloc(4 * at, np.int32)
    d_sum = ctx.alloc(4 * n, np.int32)
    ctx.quant_batch(ctx.to_device(z["quant_in"]).ptr, d_q.ptr, d_du.ptr, d_jobs.ptr, n, d_sum.ptr)
    ctx.dequant_batch(d_q.ptr, d_dq.ptr, d_jobs.ptr, n)
    assert np.array_equal(d_q.to_host(np.int32), z["quant_lev"])
    assert np.array_equal(d_dq.to_host(np.int32), z["quant_deq"])
    assert d_sum.to_host(np.int32).tolist() == rows[:, 5].tolist()
