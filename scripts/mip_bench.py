"""Times the MIP candidates of the intra mode pre-selection of one partition level -- B square blocks x every (mode, transposed) pair (16 at 8x8, 12 above), blocks
8 .. 64, 10 bit -- on the two routes the library offers:

  (a) the existing route with the predictors of every block already resident on the device: B calls of vtmhip_intra_cand_cost_batch_dev (one per block, as the
      encoder hook of oracle/ref_shim_intra.hpp issues them), 2 launches each;
  (b) what that route needs first: the upload of the B x M x W x H predictor samples (the host's predIntraMip itself is not timed);
  (c) one vtmhip_mip_presel_batch_dev call including the upload of the B pairs of lines (block and job tables resident: they do not change with the samples).

    python scripts/mip_bench.py [--blocks 256] [--reps 7]

Clock: the host's, around work that ends in a stream synchronisation, after two warm-up rounds of every side; the three sides alternate, `reps` times; median,
min and max.  (a) and (c) are also given as device time (events on the stream around the calls), which leaves the host's launch cost out.  The predictors of (a)
come from vtmhip_mip_pred_batch_dev, and the (SAD, SATD) pairs of the two routes are compared in full at every size.  The matrices are the recorded ones of
tests/golden/mip.npz.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vtm_amd.device import Context, struct_array_to_numpy  # noqa: E402
from vtm_amd.lib import IntraBlock, MipJob  # noqa: E402

BD = 10
STRIDE = 4096


def stats(v):
    return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=str, default="8,16,32,64")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    g = np.load(os.path.join(ROOT, "tests", "golden", "mip.npz"))
    ctx = Context(0)
    ctx.mip_set_tables(g["m4x4"], g["m8x8"], g["m16x16"])
    B = a.blocks
    res = dict(metric="mip_bench", blocks=B, bitDepth=BD, reps=a.reps, clock="host clock around calls + stream sync (us); *_dev_us: device events", sizes={})
    for s in [int(v) for v in a.sizes.split(",")]:
        cands = [(m, t) for t in (0, 1) for m in range(8 if s == 8 else 6)]
        M, per_row = len(cands), STRIDE // s
        rows = (B + per_row - 1) // per_row
        plane = rng.integers(0, 1 << BD, (rows * s, STRIDE)).astype(np.int16)
        line_len = 4 * s + 2                                     # the block's two lines as the regular modes need them; MIP reads top[1 .. s] and left[1 .. s]
        lines = rng.integers(0, 1 << BD, B * line_len).astype(np.int16)
        blk_arr, job_arr = (IntraBlock * B)(), (MipJob * (B * M))()
        org_off = [(b // per_row) * s * STRIDE + (b % per_row) * s for b in range(B)]
        for b in range(B):
            blk_arr[b] = IntraBlock(b * line_len, org_off[b], STRIDE, s, s, BD, 0)
            for k, (m, t) in enumerate(cands):
                job_arr[b * M + k] = MipJob((b * M + k) * s * s, b, m, t)
        n, pred_len = B * M, B * M * s * s
        d_org, d_blk, d_job = ctx.to_device(plane), ctx.to_device(struct_array_to_numpy(blk_arr)), ctx.to_device(struct_array_to_numpy(job_arr))
        d_lines, d_pred = ctx.to_device(lines), ctx.alloc(2 * pred_len)
        d_dist_a, d_dist_c = ctx.alloc(16 * n), ctx.alloc(16 * n)
        ctx.mip_pred_batch(d_lines.ptr, d_blk.ptr, B, d_job.ptr, n, d_pred.ptr)       # the predictors of route (a)
        ctx.sync()
        preds = d_pred.to_host(np.int16)
        L = ctx.L

        def route_a():
            for b in range(B):
                ctx._check(L.vtmhip_intra_cand_cost_batch_dev(ctx.h, d_org.ptr, org_off[b], STRIDE, d_pred.ptr, b * M * s * s, M, s, s, d_dist_a.ptr + 16 * M * b))

        def upload_preds():
            d_pred.upload(preds)

        def route_c():
            d_lines.upload(lines)
            ctx.mip_presel_batch(d_lines.ptr, d_org.ptr, d_blk.ptr, B, d_job.ptr, n, d_dist_c.ptr)

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
        res["sizes"]["%dx%d" % (s, s)] = dict(jobs=n, cands_per_block=M, predictor_bytes=2 * pred_len, line_bytes=int(lines.nbytes), a_cand_cost_calls_us=stats(t["a"]),
                                              b_predictor_upload_us=stats(t["b"]), c_presel_with_line_upload_us=stats(t["c"]), a_dev_us=stats(t["a_dev"]),
                                              c_dev_us=stats(t["c_dev"]), c_dev_ns_per_job=round(1000.0 * med["c_dev"] / n, 1),
                                              a_plus_b_over_c=round((med["a"] + med["b"]) / med["c"], 2), a_over_c=round(med["a"] / med["c"], 2), results_equal=True)
        for d in (d_org, d_blk, d_job, d_lines, d_pred, d_dist_a, d_dist_c):
            d.free()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
