"""Times one full-RD level of the intra chroma search -- B square chroma blocks x (4 regular modes + LM) predictions x the candidates Cb DCT2, Cr DCT2 and the three
joint Cb-Cr masks with DCT2; blocks 4 .. 32, 10 bit, base QP 32, chroma adj 3277 -- on the two routes the library offers:

  (a) the route before vtmhip_intra_chroma_chain_batch_dev, for the same jobs: vtmhip_intra_chroma_pred_batch_dev, vtmhip_subtract_batch_dev,
      vtmhip_tu_chain_crs_batch_dev and vtmhip_jccr_chain_crs_batch_dev (uniformSize = 1: the caller knows its level has one shape), the download of the predictions
      and of the reconstructed residuals, then reconstruction, clip and SSE in numpy (the original blocks are gathered once, outside the clock);
  (c) the one new call and the download of its result records.

    python scripts/intra_chroma_chain_bench.py [--blocks 256] [--reps 7]

Both routes start with the upload of the B x 2 pairs of lines; the luma plane and the block and job tables are resident.  Clock: the host's, around work that ends in
a stream synchronisation, after two warm-up rounds of every side; the sides alternate, `reps` times; median, min and max.  Device time: events on the stream around
each of the four device steps of (a) and around the call of (c) -- the latter spans the read-back of the tables and their check on the host, during which the device
idles -- and, from vtmhip_kernel_timing in a pass of its own, the kernels of (c) one by one.  Predictions, residuals, levels, reconstructions and every result field
of the two routes are compared in full at every size.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vtm_amd import lib  # noqa: E402
from vtm_amd.device import Context, intra_chroma_chain_make_jobs, struct_array_to_numpy  # noqa: E402
from vtm_amd.lib import IntraChromaBlock, IntraChromaJob, IntraChromaJointJob, IntraChromaTuJob, PelOpJob  # noqa: E402

BD, QP, ADJ = 10, 32, 3277
STRIDE = 4096
MODES = (0, 1, 18, 50, 67)
KERNELS = ("intra_chroma_resi_kernel", "intra_chroma_chain_expand_kernel", "tu_chain_lane_kernel", "tu_chain_uni_kernel", "jccr_chain_lane_kernel",
           "jccr_chain_uni_kernel", "intra_chroma_chain_finish_kernel")
RESULT = np.dtype([("sse", "<u8"), ("sseResi", "<u8"), ("sumAbs", "<i4"), ("absSum", "<i4")])
JRESULT = np.dtype([("sseCb", "<u8"), ("sseCr", "<u8"), ("sseResiCb", "<u8"), ("sseResiCr", "<u8"), ("fwdDist", "<i8"), ("sumAbs", "<i4"), ("absSum", "<i4")])
TU_RES = np.dtype([("sse", "<u8"), ("sumAbs", "<i4"), ("absSum", "<i4")])
JCCR_RES = np.dtype([("sseCb", "<u8"), ("sseCr", "<u8"), ("fwdDist", "<i8"), ("sumAbs", "<i4"), ("absSum", "<i4")])


def stats(v):
    return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=str, default="4,8,16,32")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    ctx = Context(0)
    B = a.blocks
    per, rem = divmod(QP + 6 * (BD - 8), 6)
    res = dict(metric="intra_chroma_chain_bench", blocks=B, bitDepth=BD, qp=QP, chromaAdj=ADJ, reps=a.reps,
               clock="host clock around calls + stream sync (us); *_dev_us: device events", sizes={})
    for s in [int(v) for v in a.sizes.split(",")]:
        area, per_row = s * s, STRIDE // s
        rows = ((B + per_row - 1) // per_row) * s
        plane = rng.integers(0, 1 << BD, (2 * rows, STRIDE)).astype(np.int16)           # the Cb rows, then the Cr rows
        cell, cells_per_row = 2 * s + 4, 32                                               # luma: the co-located block with three samples above and to the left
        luma = rng.integers(0, 1 << BD, (((B + cells_per_row - 1) // cells_per_row) * cell, cells_per_row * cell)).astype(np.int16)
        line_len = 4 * s + 2
        lines = rng.integers(0, 1 << BD, 2 * B * line_len).astype(np.int16)
        n_pred = B * len(MODES)
        n_tu, n_joint = 2 * n_pred, 3 * n_pred
        n_out = n_tu + n_joint
        blk_arr, pj, tj, jj, sj = (IntraChromaBlock * B)(), (IntraChromaJob * n_pred)(), (IntraChromaTuJob * n_tu)(), (IntraChromaJointJob * n_joint)(), (PelOpJob * (2 * n_pred))()
        org_off = [[c * rows * STRIDE + (b // per_row) * s * STRIDE + (b % per_row) * s for b in range(B)] for c in (0, 1)]
        for b in range(B):
            luma_off = ((b // cells_per_row) * cell + 3) * luma.shape[1] + (b % cells_per_row) * cell + 3
            blk_arr[b] = IntraChromaBlock(2 * b * line_len, (2 * b + 1) * line_len, org_off[0][b], org_off[1][b], luma_off, STRIDE, luma.shape[1], s, s, 0, 0, BD, 1, 1, 0, 0)
            for k, mode in enumerate(MODES):
                p = b * len(MODES) + k
                pj[p] = IntraChromaJob(2 * p * area, (2 * p + 1) * area, b, mode)
        pred_block = np.array([j.block for j in pj])
        for p in range(n_pred):
            for c in (0, 1):
                sj[2 * p + c] = PelOpJob(org_off[c][pred_block[p]], (2 * p + c) * area, (2 * p + c) * area, STRIDE, s, s, s, s, BD, 0, 0, 0, 0)
                tj[2 * p + c] = IntraChromaTuJob((2 * p + c) * area, p, per, rem, c, lib.DCT2, 0, 0, ADJ, 0)
            for m in (1, 2, 3):
                jj[3 * p + m - 1] = IntraChromaJointJob((n_tu + 3 * p + m - 1) * area, p, per, rem, lib.DCT2, 0, m, 0, ADJ, 0)
        tu_pred, tu_comp, joint_pred = np.array([t.pred for t in tj]), np.array([t.component for t in tj]), np.array([t.pred for t in jj])
        xt, xj, plan_t, plan_j, crs = intra_chroma_chain_make_jobs(blk_arr, pj, tj, jj)
        assert plan_t == (s, s, 1) and plan_j == (s, s, 1) and crs == 1
        org = [np.stack([plane[o // STRIDE:o // STRIDE + s, o % STRIDE:o % STRIDE + s].reshape(-1) for o in org_off[c]]).astype(np.int64) for c in (0, 1)]
        s2n = struct_array_to_numpy
        d_org, d_luma, d_lines, d_blk, d_pj, d_tj, d_jj, d_sj, d_xt, d_xj = (ctx.to_device(v) for v in (plane, luma, lines, s2n(blk_arr), s2n(pj), s2n(tj), s2n(jj), s2n(sj),
                                                                                                     s2n(xt), s2n(xj)))
        sizes_a = (4 * n_pred * area, 4 * n_pred * area, 4 * n_out * area, 2 * n_out * area, 2 * n_out * area, 16 * n_tu, 32 * n_joint)
        sizes_c = sizes_a[:5] + (24 * n_tu, 48 * n_joint)
        d_pred_a, d_resi_a, d_lev_a, d_rec_a, d_reccr_a, d_res_a, d_jres_a = (ctx.to_device(np.zeros(n, np.uint8)) for n in sizes_a)
        d_pred_c, d_resi_c, d_lev_c, d_rec_c, d_reccr_c, d_res_c, d_jres_c = (ctx.to_device(np.zeros(n, np.uint8)) for n in sizes_c)
        out = {}

        def a_pred():
            ctx.intra_chroma_pred_batch(d_lines.ptr, d_luma.ptr, d_blk.ptr, B, d_pj.ptr, n_pred, d_pred_a.ptr)

        def a_sub():
            ctx.subtract_batch(d_org.ptr, d_pred_a.ptr, d_resi_a.ptr, d_sj.ptr, 2 * n_pred)

        def a_chain():
            ctx.tu_chain_crs_batch(d_resi_a.ptr, d_xt.ptr, n_tu, s, s, d_res_a.ptr, d_lev_a.ptr, d_rec_a.ptr, uniform=True)

        def a_joint():
            ctx.jccr_chain_crs_batch(d_resi_a.ptr, d_xj.ptr, n_joint, s, s, d_jres_a.ptr, d_lev_a.ptr, d_rec_a.ptr, d_reccr_a.ptr, uniform=True)

        def finish(pred, rec, orig):
            reco = np.clip(pred.astype(np.int32) + rec, 0, (1 << BD) - 1)
            d = orig - reco
            return reco.astype(np.int16), (d * d).sum(1).astype(np.uint64)

        def route_a():
            d_lines.upload(lines)
            a_pred()
            a_sub()
            a_chain()
            a_joint()
            pred = d_pred_a.to_host(np.int16, shape=(n_pred, 2, area))
            rec = d_rec_a.to_host(np.int16, shape=(n_out, area))
            rec_cr = d_reccr_a.to_host(np.int16, shape=(n_out, area))
            blk_t, blk_j = pred_block[tu_pred], pred_block[joint_pred]
            org_t = np.where(tu_comp[:, None] == 0, org[0][blk_t], org[1][blk_t])
            out["a"] = (finish(pred[tu_pred, tu_comp], rec[:n_tu], org_t), finish(pred[joint_pred, 0], rec[n_tu:], org[0][blk_j]),
                        finish(pred[joint_pred, 1], rec_cr[n_tu:], org[1][blk_j]))

        def c_call():
            ctx.intra_chroma_chain_batch(d_lines.ptr, d_luma.ptr, d_org.ptr, d_blk.ptr, B, d_pj.ptr, n_pred, d_tj.ptr, n_tu, d_jj.ptr, n_joint, d_pred_c.ptr, d_resi_c.ptr,
                                         d_rec_c.ptr, d_reccr_c.ptr, d_res_c.ptr, d_jres_c.ptr, d_lev_c.ptr)

        def route_c():
            d_lines.upload(lines)
            c_call()
            out["c"] = (np.frombuffer(d_res_c.to_host(np.uint8, shape=(-1,)).tobytes(), RESULT), np.frombuffer(d_jres_c.to_host(np.uint8, shape=(-1,)).tobytes(), JRESULT))

        def wall(fn):
            ctx.sync()
            t = time.perf_counter()
            fn()
            ctx.sync()
            return (time.perf_counter() - t) * 1e6

        def dev(fn):
            ctx.timer_start()
            fn()
            return ctx.timer_stop_ms() * 1000.0

        for _ in range(2):
            route_a()
            route_c()
        ctx.sync()
        steps = (("a_pred_dev", a_pred), ("a_sub_dev", a_sub), ("a_chain_dev", a_chain), ("a_joint_dev", a_joint), ("c_dev", c_call))
        t = {k: [] for k in ("a", "c") + tuple(k for k, _ in steps)}
        for _ in range(a.reps):
            t["a"].append(wall(route_a))
            t["c"].append(wall(route_c))
            for k, fn in steps:
                t[k].append(dev(fn))
        ctx.kernel_timing(True)
        for _ in range(a.reps):
            c_call()
        split = {k: round(1000.0 * ctx.kernel_timing_read(k)[0] / a.reps, 1) for k in KERNELS}
        ctx.kernel_timing(False)
        # the two routes in full
        (reco_t, sse_t), (reco_cb, sse_cb), (reco_cr, sse_cr) = out["a"]
        rc, jc = out["c"]
        rec_c, reccr_c = d_rec_c.to_host(np.int16, shape=(n_out, area)), d_reccr_c.to_host(np.int16, shape=(n_out, area))
        same = (np.array_equal(d_pred_a.to_host(np.int16, shape=(-1,)), d_pred_c.to_host(np.int16, shape=(-1,)))
                and np.array_equal(d_resi_a.to_host(np.int16, shape=(-1,)), d_resi_c.to_host(np.int16, shape=(-1,)))
                and np.array_equal(d_lev_a.to_host(np.int32, shape=(-1,)), d_lev_c.to_host(np.int32, shape=(-1,)))
                and np.array_equal(reco_t, rec_c[:n_tu]) and np.array_equal(reco_cb, rec_c[n_tu:]) and np.array_equal(reco_cr, reccr_c[n_tu:])
                and np.array_equal(sse_t, rc["sse"]) and np.array_equal(sse_cb, jc["sseCb"]) and np.array_equal(sse_cr, jc["sseCr"]))
        ra = np.frombuffer(d_res_a.to_host(np.uint8, shape=(-1,)).tobytes(), TU_RES)
        ja = np.frombuffer(d_jres_a.to_host(np.uint8, shape=(-1,)).tobytes(), JCCR_RES)
        same = same and all(np.array_equal(ra[k], rc[q]) for k, q in (("sse", "sseResi"), ("sumAbs", "sumAbs"), ("absSum", "absSum")))
        same = same and all(np.array_equal(ja[k], jc[q]) for k, q in (("sseCb", "sseResiCb"), ("sseCr", "sseResiCr"), ("fwdDist", "fwdDist"), ("sumAbs", "sumAbs"),
                                                                       ("absSum", "absSum")))
        assert same, "the two routes disagree at %dx%d" % (s, s)
        med = {k: float(np.median(v)) for k, v in t.items()}
        a_dev_sum = med["a_pred_dev"] + med["a_sub_dev"] + med["a_chain_dev"] + med["a_joint_dev"]
        reco_all = np.concatenate([reco_t.reshape(-1), reco_cb.reshape(-1), reco_cr.reshape(-1)])
        res["sizes"]["%dx%d" % (s, s)] = dict(predictions=n_pred, single_jobs=n_tu, joint_jobs=n_joint, download_bytes_a=2 * (2 * n_pred + n_tu + 2 * n_joint) * area,
                                              download_bytes_c=24 * n_tu + 48 * n_joint, a_us=stats(t["a"]), c_us=stats(t["c"]), a_over_c=round(med["a"] / med["c"], 2),
                                              a_pred_dev_us=stats(t["a_pred_dev"]), a_sub_dev_us=stats(t["a_sub_dev"]), a_chain_dev_us=stats(t["a_chain_dev"]),
                                              a_joint_dev_us=stats(t["a_joint_dev"]), a_dev_sum_us=round(a_dev_sum, 1), c_dev_us=stats(t["c_dev"]), c_kernels_us=split,
                                              c_kernels_sum_us=round(sum(split.values()), 1), coded_single=int((rc["absSum"] > 0).sum()), coded_joint=int((jc["absSum"] > 0).sum()),
                                              clipped_samples=int((reco_all == 0).sum() + (reco_all == (1 << BD) - 1).sum()), results_equal=True)
        for d in (d_org, d_luma, d_lines, d_blk, d_pj, d_tj, d_jj, d_sj, d_xt, d_xj, d_pred_a, d_resi_a, d_lev_a, d_rec_a, d_reccr_a, d_res_a, d_jres_a, d_pred_c, d_resi_c,
                  d_lev_c, d_rec_c, d_reccr_c, d_res_c, d_jres_c):
            d.free()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
