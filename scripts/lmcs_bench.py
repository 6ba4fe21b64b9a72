"""Times the chains with LMCS chroma residual scaling (vtmhip_tu_chain_crs_batch_dev, vtmhip_jccr_chain_crs_batch_dev) against their plain counterparts on
the TU set of scripts/jccr_bench.py: the 4:2:0 chroma TUs of a 64 / 32 / 16 / 8 luma quadtree of one 1920x1088 picture -- 510 + 2040 + 8160 + 32640 pairs of
32x32 / 16x16 / 8x8 / 4x4 -- each level one uniform launch (the plain chain: 2 n jobs, Cb then Cr; the joint chain: n pairs).  The adj of a TU is drawn from
256 .. 16384.  Device events around a run of calls after warm-up; the CRS call and the plain call alternate within the process, the pair is repeated; the
kernels' own time comes from vtmhip_kernel_timing in a run of its own (the joint calls read their job table back before they launch).
Also: the mapped-domain luma residual and reconstruction (vtmhip_lmcs_resi_batch_dev / vtmhip_lmcs_reco_batch_dev) over the picture's luma CUs per quadtree
level, with the achieved bytes/s (two sample reads and one write per sample) against the 8 TB/s HBM peak of the MI355X.

    python scripts/lmcs_bench.py [--reps 9] [--iters 20]

One more pair: 16x4 TUs on the generic LDS kernel (64 threads per TU), whose CRS form runs at 4 instead of 5 waves per SIMD.

Prints one JSON line: us per level (median, min, max over the repetitions) for every side and the ratios CRS / plain."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import lmcs_util as lu  # noqa: E402
from vtm_amd import lib  # noqa: E402
from vtm_amd.device import Context  # noqa: E402

CW, CH, BD, QP = 960, 544, 10, 32 + 12
LW, LH = 1920, 1088
MASKS = [(3, 0), (2, 0), (1, 0), (3, 1), (2, 1), (1, 1)]   # (cbfMask, signFlag): all six joint modes in turn
HBM_PEAK = 8.0e12                                          # bytes/s


def stats(v):
    return dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    cb = rng.integers(-60, 61, (CH, CW)).astype(np.int16)
    cr = np.clip(cb.astype(np.int32) * 3 // 4 + rng.integers(-15, 16, (CH, CW)), -1023, 1023).astype(np.int16)
    ctx = Context(0)
    d_resi = ctx.to_device(np.concatenate([cb.reshape(-1), cr.reshape(-1)]))
    d_lv = ctx.alloc(4 * 2 * CW * CH)
    res = dict(metric="lmcs_bench", picture="1920x1088 4:2:0", bitDepth=BD, qp=QP - 12, reps=a.reps, iters=a.iters, levels={}, luma={})

    def timed(fn):
        ctx.timer_start()
        for _ in range(a.iters):
            fn()
        return ctx.timer_stop_ms() * 1000.0 / a.iters

    def alternate(f, g):
        for _ in range(3):   # warm-up
            f()
            g()
        ctx.sync()
        tf, tg = [], []
        for _ in range(a.reps):
            tf.append(timed(f))
            tg.append(timed(g))
        return tf, tg

    def kernels(f, g, kf, kg):
        ctx.kernel_timing(True)
        for _ in range(a.iters):
            f()
        msf, nf = ctx.kernel_timing_read(kf)
        ctx.kernel_timing(False)
        ctx.kernel_timing(True)
        for _ in range(a.iters):
            g()
        msg, ng = ctx.kernel_timing_read(kg)
        ctx.kernel_timing(False)
        assert nf == a.iters and ng == a.iters
        return msf * 1000.0 / nf, msg * 1000.0 / ng

    for s in (32, 16, 8, 4):
        pos = [(y, x) for y in range(0, CH, s) for x in range(0, CW, s)]
        n = len(pos)
        adj = rng.integers(256, 16385, n)
        jj, tj = (lib.JccrJob * n)(), (lib.TuJob * (2 * n))()
        for k, (y, x) in enumerate(pos):
            j = jj[k]
            j.cbOff, j.crOff, j.outOff, j.resiStride, j.width, j.height = y * CW + x, CW * CH + y * CW + x, k * s * s, CW, s, s
            j.qpPer, j.qpRem, j.typeHor, j.bitDepth, j.isIRAP, j.chromaAdj = QP // 6, QP % 6, lib.DCT2, BD, 0, int(adj[k])
            j.cbfMask, j.signFlag = MASKS[k % 6]
            for c in range(2):
                t = tj[c * n + k]
                t.resiOff, t.outOff, t.resiStride, t.width, t.height = c * CW * CH + y * CW + x, (c * n + k) * s * s, CW, s, s
                t.qpPer, t.qpRem, t.typeHor, t.typeVer, t.bitDepth, t.isIRAP, t.chromaAdj = QP // 6, QP % 6, lib.DCT2, lib.DCT2, BD, 0, int(adj[k])
        d_jj, d_tj = ctx.to_device(np.frombuffer(jj, np.uint8).copy()), ctx.to_device(np.frombuffer(tj, np.uint8).copy())
        d_rj, d_rt = ctx.alloc(C.sizeof(lib.JccrResult) * n), ctx.alloc(C.sizeof(lib.TuResult) * 2 * n)

        def tu_crs():
            ctx.tu_chain_crs_batch(d_resi.ptr, d_tj.ptr, 2 * n, s, s, d_rt.ptr, d_lv.ptr, None, uniform=True)

        def tu_plain():
            ctx.tu_chain_batch(d_resi.ptr, d_tj.ptr, 2 * n, s, s, d_rt.ptr, d_lv.ptr, None, uniform=True)

        def jc_crs():
            ctx.jccr_chain_crs_batch(d_resi.ptr, d_jj.ptr, n, s, s, d_rj.ptr, d_lv.ptr, None, None, uniform=True)

        def jc_plain():
            ctx.jccr_chain_batch(d_resi.ptr, d_jj.ptr, n, s, s, d_rj.ptr, d_lv.ptr, None, None, uniform=True)

        kname = "lane" if s == 4 else "uni"
        t_tc, t_tp = alternate(tu_crs, tu_plain)
        t_jc, t_jp = alternate(jc_crs, jc_plain)
        k_tc, k_tp = kernels(tu_crs, tu_plain, "tu_chain_%s_kernel" % kname, "tu_chain_%s_kernel" % kname)
        k_jc, k_jp = kernels(jc_crs, jc_plain, "jccr_chain_%s_kernel" % kname, "jccr_chain_%s_kernel" % kname)
        # spot check: a few TUs and pairs of the CRS runs against the expectation composed from the restatement and the oracle
        tu_crs()
        jc_crs()
        got_t = (lib.TuResult * (2 * n)).from_buffer_copy(d_rt.to_host(np.uint8).tobytes())
        got_j = (lib.JccrResult * n).from_buffer_copy(d_rj.to_host(np.uint8).tobytes())
        for k in range(0, n, max(1, n // 5)):
            y, x = pos[k]
            e = lu.tu_chain_expect(cb[y:y + s, x:x + s], int(adj[k]), BD, QP // 6, QP % 6, 0, False)
            assert (got_t[k].sse, got_t[k].sumAbs, got_t[k].absSum) == (e["sse"], e["sumAbs"], e["absSum"]), (s, k)
            e = lu.jccr_chain_expect(cb[y:y + s, x:x + s], cr[y:y + s, x:x + s], int(adj[k]), jj[k].cbfMask, jj[k].signFlag, BD, QP // 6, QP % 6, 0, False)
            assert (got_j[k].sseCb, got_j[k].sseCr, got_j[k].fwdDist, got_j[k].sumAbs, got_j[k].absSum) == (e["sseCb"], e["sseCr"], e["fwdDist"], e["sumAbs"], e["absSum"]), (s, k)
        res["levels"]["%dx%d" % (s, s)] = dict(
            pairs=n, plain_chain=dict(crs_us=stats(t_tc), plain_us=stats(t_tp), ratio=round(float(np.median(t_tc) / np.median(t_tp)), 3), crs_kernel_us=round(k_tc, 2),
                                      plain_kernel_us=round(k_tp, 2), kernel_ratio=round(k_tc / k_tp, 3)),
            joint_chain=dict(crs_us=stats(t_jc), plain_us=stats(t_jp), ratio=round(float(np.median(t_jc) / np.median(t_jp)), 3), crs_kernel_us=round(k_jc, 2),
                             plain_kernel_us=round(k_jp, 2), kernel_ratio=round(k_jc / k_jp, 3)))

    # the generic LDS kernel (64 threads per TU), which takes the 4-sample-side and transform-skip chroma jobs: 16x4 TUs of the Cb plane, one uniform launch
    # (uniform shapes other than 4x4 / 8x4 / 4x8 and sides >= 8 go to the generic kernel).  Call times only: that launch has no kernel timer.
    w, h = 16, 4
    pos = [(y, x) for y in range(0, CH, h) for x in range(0, CW, w)]
    n = len(pos)
    adj = rng.integers(256, 16385, n)
    tj = (lib.TuJob * n)()
    for k, (y, x) in enumerate(pos):
        t = tj[k]
        t.resiOff, t.outOff, t.resiStride, t.width, t.height = y * CW + x, k * w * h, CW, w, h
        t.qpPer, t.qpRem, t.typeHor, t.typeVer, t.bitDepth, t.isIRAP, t.chromaAdj = QP // 6, QP % 6, lib.DCT2, lib.DCT2, BD, 0, int(adj[k])
    d_tj, d_rt = ctx.to_device(np.frombuffer(tj, np.uint8).copy()), ctx.alloc(C.sizeof(lib.TuResult) * n)

    def gen_crs():
        ctx.tu_chain_crs_batch(d_resi.ptr, d_tj.ptr, n, w, h, d_rt.ptr, d_lv.ptr, None, uniform=True)

    def gen_plain():
        ctx.tu_chain_batch(d_resi.ptr, d_tj.ptr, n, w, h, d_rt.ptr, d_lv.ptr, None, uniform=True)

    t_gc, t_gp = alternate(gen_crs, gen_plain)
    gen_crs()
    got_t = (lib.TuResult * n).from_buffer_copy(d_rt.to_host(np.uint8).tobytes())
    for k in range(0, n, max(1, n // 5)):
        y, x = pos[k]
        e = lu.tu_chain_expect(cb[y:y + h, x:x + w], int(adj[k]), BD, QP // 6, QP % 6, 0, False)
        assert (got_t[k].sse, got_t[k].sumAbs, got_t[k].absSum) == (e["sse"], e["sumAbs"], e["absSum"]), ("16x4", k)
    res["generic_16x4"] = dict(tus=n, crs_us=stats(t_gc), plain_us=stats(t_gp), ratio=round(float(np.median(t_gc) / np.median(t_gp)), 3))

    # the luma ops over the picture's CUs, level by level
    lut = lu.make_lut(7, BD)
    ctx.set_lmcs_fwd_lut(lut, BD)
    org, pred = rng.integers(0, 1 << BD, (LH, LW)).astype(np.int16), rng.integers(0, 1 << BD, (LH, LW)).astype(np.int16)
    d_org, d_pred, d_res, d_rec = ctx.to_device(org), ctx.to_device(pred), ctx.alloc(2 * LW * LH), ctx.alloc(2 * LW * LH)
    for s in (64, 32, 16, 8):
        pos = [(y, x) for y in range(0, LH, s) for x in range(0, LW, s)]
        n = len(pos)
        lj = (lib.LmcsJob * n)()
        for k, (y, x) in enumerate(pos):
            j = lj[k]
            j.orgOff = j.predOff = j.resiOff = j.dstOff = y * LW + x
            j.orgStride = j.predStride = j.resiStride = j.dstStride = LW
            j.width, j.height, j.bitDepth, j.flags = s, s, BD, lib.LMCS_MAP_PRED
        d_lj = ctx.to_device(np.frombuffer(lj, np.uint8).copy())

        def resi():
            ctx.lmcs_resi_batch(d_org.ptr, d_pred.ptr, d_res.ptr, d_lj.ptr, n)

        def reco():
            ctx.lmcs_reco_batch(d_pred.ptr, d_res.ptr, d_rec.ptr, d_lj.ptr, n)

        t_rs, t_rc = alternate(resi, reco)
        r, _ = lu.resi_expect(org, pred, lut, True)
        assert np.array_equal(d_res.to_host(np.int16).reshape(LH, LW), r)
        assert np.array_equal(d_rec.to_host(np.int16).reshape(LH, LW), lu.reco_expect(pred, r, lut, True, BD))
        nbytes = 3 * 2 * LW * LH
        res["luma"]["%dx%d" % (s, s)] = dict(cus=n, resi_us=stats(t_rs), reco_us=stats(t_rc), resi_GBps=round(nbytes / np.median(t_rs) / 1e3, 1),
                                             reco_GBps=round(nbytes / np.median(t_rc) / 1e3, 1), resi_share_of_hbm_peak=round(nbytes / np.median(t_rs) * 1e6 / HBM_PEAK, 4),
                                             reco_share_of_hbm_peak=round(nbytes / np.median(t_rc) * 1e6 / HBM_PEAK, 4))
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
