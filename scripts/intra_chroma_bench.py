"""Times the chroma mode pre-selection of IntraSearch::estIntraPredChromaQT for one partition level -- B blocks x the candidates the reference pre-selects over
(DC, HOR, VER and both MDLM modes: the regular candidates except planar and DM, LM is kept without a check), square chroma blocks 4 .. 32, 10 bit, above and left
available with full above-right and below-left reach, the default (not collocated) down-sampling -- on the two routes the library offers:

  (a) the route of the parent commit with the Cb and Cr predictors of every block already resident on the device: 2 B calls of
      vtmhip_intra_cand_cost_batch_dev (one per block and component), 2 launches each;
  (b) what that route needs first: the upload of the B x 2 x 5 x W x H predictor samples (their formation on the host is not timed);
  (c) one vtmhip_intra_chroma_presel_batch_dev call including the upload of the 2 B pairs of lines and of the block and job tables.  The luma reconstruction and
      the originals are resident in both routes.

    python scripts/intra_chroma_bench.py [--blocks 256] [--reps 7]

Clock: the host's, around work that ends in a stream synchronisation, after two warm-up rounds of every side; the three sides alternate, `reps` times; median,
min and max.  (a) and (c) are also given as device time (events on the stream around the calls).  The predictors of (a) come from
vtmhip_intra_chroma_pred_batch_dev, and the four distortions per job of the two routes are compared in full at every size.
luma_*: the down-sampling's traffic per call from the block table -- unique_bytes: the luma samples the staged extent covers (inner 2W x 2H, three rows above over
2 (W + H) + 3 columns, three columns left over 2 (H + W) rows), load_bytes: what the lanes request (six 2-byte loads per down-sampled sample) -- and both over the
fused call's device time.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vtm_amd import device  # noqa: E402
from vtm_amd.device import Context, struct_array_to_numpy  # noqa: E402

BD = 10
MODES = [1, 18, 50, 68, 69]
LUMA_STRIDE, ORG_STRIDE = 4096, 2048


def stats(v):
    return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=str, default="4,8,16,32")
    a = ap.parse_args()
    rng = np.random.default_rng(6)
    ctx = Context(0)
    B, M = a.blocks, len(MODES)
    res = dict(metric="intra_chroma_bench", blocks=B, modes=MODES, bitDepth=BD, reps=a.reps, clock="host clock around calls + stream sync (us); *_dev_us: device events", sizes={})
    for s in [int(v) for v in a.sizes.split(",")]:
        cell = 4 * s + 8                                  # luma: three samples of margin, the block and its above-right / below-left reach
        per_row = LUMA_STRIDE // cell
        rows = (B + per_row - 1) // per_row
        luma = rng.integers(0, 1 << BD, (rows * cell, LUMA_STRIDE)).astype(np.int16)
        org_per_row = ORG_STRIDE // s
        org_rows = (B + org_per_row - 1) // org_per_row * s
        org = rng.integers(0, 1 << BD, (2 * org_rows, ORG_STRIDE)).astype(np.int16)     # Cb rows, then Cr rows
        blocks = []
        for b in range(B):
            lines = []
            for c in (0, 1):
                line = rng.integers(0, 1 << BD, 4 * s + 2).astype(np.int16)
                line[2 * s + 1] = line[0]
                lines.append((line[:2 * s + 1], line[2 * s + 1:]))
            cb_off = (b // org_per_row) * s * ORG_STRIDE + (b % org_per_row) * s
            blocks.append(dict(w=s, h=s, bd=BD, above=1, left=1, ar=s, bl=s, first_row=0, coloc=0, lines=lines, modes=MODES,
                               luma_off=((b // per_row) * cell + 4) * LUMA_STRIDE + (b % per_row) * cell + 4, luma_stride=LUMA_STRIDE,
                               org_off=(cb_off, cb_off + org_rows * ORG_STRIDE), org_stride=ORG_STRIDE))
        (blk_arr, job_arr, n), lines, pred_len = device.pack_intra_chroma_tables(blocks)
        assert n == B * M and pred_len == 2 * n * s * s
        for k, j in enumerate(job_arr):                   # route (a) wants the M predictors of one (block, component) next to each other
            b, m = divmod(k, M)
            j.cbPredOff, j.crPredOff = ((2 * b) * M + m) * s * s, ((2 * b + 1) * M + m) * s * s
        blk_np, job_np = struct_array_to_numpy(blk_arr), struct_array_to_numpy(job_arr)
        d_luma, d_org, d_blk, d_job = ctx.to_device(luma), ctx.to_device(org), ctx.to_device(blk_np), ctx.to_device(job_np)
        d_lines, d_pred = ctx.to_device(lines), ctx.alloc(2 * pred_len)
        d_dist_a, d_dist_c = ctx.alloc(32 * n), ctx.alloc(32 * n)
        ctx.intra_chroma_pred_batch(d_lines.ptr, d_luma.ptr, d_blk.ptr, B, d_job.ptr, n, d_pred.ptr)       # the predictors of route (a)
        ctx.sync()
        preds = d_pred.to_host(np.int16)
        L = ctx.L

        def route_a():
            for b in range(B):
                for c in (0, 1):
                    ctx._check(L.vtmhip_intra_cand_cost_batch_dev(ctx.h, d_org.ptr, blocks[b]["org_off"][c], ORG_STRIDE, d_pred.ptr, (2 * b + c) * M * s * s, M, s, s,
                                                                  d_dist_a.ptr + 16 * M * (2 * b + c)))

        def upload_preds():
            d_pred.upload(preds)

        def route_c():
            d_lines.upload(lines)
            d_blk.upload(blk_np)
            d_job.upload(job_np)
            ctx.intra_chroma_presel_batch(d_lines.ptr, d_luma.ptr, d_org.ptr, d_blk.ptr, B, d_job.ptr, n, d_dist_c.ptr)

        def kernel_c():
            ctx.intra_chroma_presel_batch(d_lines.ptr, d_luma.ptr, d_org.ptr, d_blk.ptr, B, d_job.ptr, n, d_dist_c.ptr)

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

        sides = dict(a=route_a, b=upload_preds, c=route_c)
        for _ in range(2):
            for fn in sides.values():
                fn()
        ctx.sync()
        t = {k: [] for k in ("a", "b", "c", "a_dev", "c_dev", "c_kernels_dev")}
        for _ in range(a.reps):
            for k, fn in sides.items():
                t[k].append(wall(fn))
            t["a_dev"].append(dev(route_a))
            t["c_dev"].append(dev(route_c))
            t["c_kernels_dev"].append(dev(kernel_c))
        da = d_dist_a.to_host(np.uint64).reshape(B, 2, 2, M)      # per block and component: the SADs, then the SATDs
        dc = d_dist_c.to_host(np.uint64).reshape(B, M, 2, 2)      # per job: component, (SAD, SATD)
        assert np.array_equal(da.transpose(0, 3, 1, 2), dc), "the two routes disagree at %dx%d" % (s, s)
        med = {k: float(np.median(v)) for k, v in t.items()}
        ds_samples = B * (s * s + 2 * s + 2 * s)
        unique = 2 * B * (4 * s * s + 3 * (4 * s + 3) + 3 * 4 * s)
        kern_s = med["c_kernels_dev"] * 1e-6
        res["sizes"]["%dx%d" % (s, s)] = dict(jobs=n, predictor_bytes=2 * pred_len, line_bytes=int(lines.nbytes), table_bytes=int(blk_np.nbytes + job_np.nbytes),
                                              a_cand_cost_calls_us=stats(t["a"]), b_predictor_upload_us=stats(t["b"]), c_presel_with_uploads_us=stats(t["c"]),
                                              a_dev_us=stats(t["a_dev"]), c_dev_us=stats(t["c_dev"]), c_kernels_dev_us=stats(t["c_kernels_dev"]),
                                              a_plus_b_over_c=round((med["a"] + med["b"]) / med["c"], 2), a_over_c=round(med["a"] / med["c"], 2),
                                              luma_unique_bytes=unique, luma_load_bytes=12 * ds_samples, luma_unique_GBps=round(unique / kern_s / 1e9, 2),
                                              luma_load_GBps=round(12 * ds_samples / kern_s / 1e9, 2), results_equal=True)
        for d in (d_luma, d_org, d_blk, d_job, d_lines, d_pred, d_dist_a, d_dist_c):
            d.free()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
