"""Times the first-round intra mode pre-selection of one partition level -- B blocks x the 35 first-round modes (planar, DC, the even angular modes), square
blocks 8 .. 64, 10 bit, reference line 0 -- on the two routes the library offers:

  (a) the existing route with the 35 predictors of every block already resident on the device: B calls of vtmhip_intra_cand_cost_batch_dev (one per block, as
      the encoder hook of oracle/ref_shim_intra.hpp issues them), 2 launches each;
  (b) what that route needs first: the upload of the B x 35 x W x H predictor samples (the host's predIntraAng itself is not timed);
  (c) one vtmhip_intra_presel_batch_dev call including the upload of the B pairs of lines (block and job tables resident: they do not change with the samples).

    python scripts/intra_bench.py [--blocks 256] [--reps 7]

Clock: the host's, around work that ends in a stream synchronisation, after two warm-up rounds of every side; the three sides alternate, `reps` times; median,
min and max.  (a) and (c) are also given as device time (events on the stream around the calls), which leaves the host's launch cost out.  The predictors of (a)
come from vtmhip_intra_pred_batch_dev, and the (SAD, SATD) pairs of the two routes are compared in full at every size.  Prints one JSON line."""
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
MODES = [0, 1] + list(range(2, 67, 2))
STRIDE = 4096


def stats(v):
    return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=str, default="8,16,32,64")
    a = ap.parse_args()
    rng = np.random.default_rng(6)
    ctx = Context(0)
    B, M = a.blocks, len(MODES)
    res = dict(metric="intra_bench", blocks=B, modes=M, bitDepth=BD, reps=a.reps, clock="host clock around calls + stream sync (us); *_dev_us: device events", sizes={})
    for s in [int(v) for v in a.sizes.split(",")]:
        per_row = STRIDE // s
        rows = (B + per_row - 1) // per_row
        plane = rng.integers(0, 1 << BD, (rows * s, STRIDE)).astype(np.int16)
        blocks = []
        for b in range(B):
            line = rng.integers(0, 1 << BD, 4 * s + 2).astype(np.int16)
            line[2 * s + 1] = line[0]
            blocks.append(dict(w=s, h=s, bd=BD, m=0, top=line[:2 * s + 1], left=line[2 * s + 1:], modes=MODES, org_off=(b // per_row) * s * STRIDE + (b % per_row) * s,
                               org_stride=STRIDE))
        (blk_arr, job_arr, n), lines, pred_len = device.pack_intra_tables(blocks)
        assert n == B * M and pred_len == n * s * s
        d_org, d_blk, d_job = ctx.to_device(plane), ctx.to_device(struct_array_to_numpy(blk_arr)), ctx.to_device(struct_array_to_numpy(job_arr))
        d_lines, d_pred = ctx.to_device(lines), ctx.alloc(2 * pred_len)
        d_dist_a, d_dist_c = ctx.alloc(16 * n), ctx.alloc(16 * n)
        ctx.intra_pred_batch(d_lines.ptr, d_blk.ptr, B, d_job.ptr, n, d_pred.ptr)       # the predictors of route (a)
        ctx.sync()
        preds = d_pred.to_host(np.int16)
        L = ctx.L

        def route_a():
            for b in range(B):
                ctx._check(L.vtmhip_intra_cand_cost_batch_dev(ctx.h, d_org.ptr, blocks[b]["org_off"], STRIDE, d_pred.ptr, b * M * s * s, M, s, s, d_dist_a.ptr + 16 * M * b))

        def upload_preds():
            d_pred.upload(preds)

        def route_c():
            d_lines.upload(lines)
            ctx.intra_presel_batch(d_lines.ptr, d_org.ptr, d_blk.ptr, B, d_job.ptr, n, d_dist_c.ptr)

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
        t = {k: [] for k in ("a", "b", "c", "a_dev", "c_dev")}
        for _ in range(a.reps):
            for k, fn in sides.items():
                t[k].append(wall(fn))
            t["a_dev"].append(dev(route_a))
            t["c_dev"].append(dev(route_c))
        da = d_dist_a.to_host(np.uint64).reshape(B, 2, M)      # per block: the SADs, then the SATDs
        dc = d_dist_c.to_host(np.uint64).reshape(B, M, 2)
        assert np.array_equal(da.transpose(0, 2, 1), dc), "the two routes disagree at %dx%d" % (s, s)
        med = {k: float(np.median(v)) for k, v in t.items()}
        res["sizes"]["%dx%d" % (s, s)] = dict(jobs=n, predictor_bytes=2 * pred_len, line_bytes=int(lines.nbytes), a_cand_cost_calls_us=stats(t["a"]), b_predictor_upload_us=stats(t["b"]),
                                              c_presel_with_line_upload_us=stats(t["c"]), a_dev_us=stats(t["a_dev"]), c_dev_us=stats(t["c_dev"]),
                                              a_plus_b_over_c=round((med["a"] + med["b"]) / med["c"], 2), a_over_c=round(med["a"] / med["c"], 2),
                                              results_equal=True)
        for d in (d_org, d_blk, d_job, d_lines, d_pred, d_dist_a, d_dist_c):
            d.free()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
