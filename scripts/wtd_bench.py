"""Times vtmhip_sse_wtd_batch_dev (DF_SSE_WTD, luma with the fused inverse reshape) against vtmhip_dist_batch_dev in DF_SSE mode on the same blocks:
the CU-level final distortions of one 1920x1080 4:2:0 picture (coded height 1088) -- every CU of a 64x64 / 32x32 / 16x16 / 8x8 quadtree, Y + Cb + Cr,
one launch each.  Device events around a run of launches after warm-up; the two kernels alternate, the pair is repeated.

    python scripts/wtd_bench.py [--reps 9] [--iters 20] [--signal 0]

Prints one JSON line: us per picture (median, min, max over the repetitions) for both, the ratio, the algorithmic bytes (org + cur samples, plus the
co-located luma for PQ chroma) over the kernel time as a share of the 8 TB/s HBM peak, and the launch count per picture."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import wtd_util as wu  # noqa: E402
from vtm_amd import lib  # noqa: E402
from vtm_amd.device import Context  # noqa: E402

W, H = 1920, 1088
HBM_PEAK = 8.0e12


def jobs_for_picture(signal):
    wtd, sse = [], []
    cw, ch = W // 2, H // 2
    offs = (0, W * H, W * H + cw * ch)
    luma_bytes = 0
    for s in (64, 32, 16, 8):
        for y in range(0, H, s):
            for x in range(0, W, s):
                for comp in (0, 1, 2):
                    sh = 1 if comp else 0
                    bw, stride = s >> sh, (W >> sh)
                    off = offs[comp] + (y >> sh) * stride + (x >> sh)
                    wtd.append(dict(orgOff=off, curOff=off, orgLumaOff=y * W + x, orgStride=stride, curStride=stride, orgLumaStride=W, width=bw, height=bw,
                                    compID=comp, cShiftX=sh, cShiftY=sh, flags=0 if comp else lib.WTD_INV_RESHAPE_CUR))
                    sse.append((off, off, stride, stride, bw, bw, 0, lib.DIST_SSE))
                    if comp and signal != wu.SDR and signal != wu.HLG:
                        luma_bytes += bw * bw * 2
    sse_arr = (lib.DistJob * len(sse))(*[lib.DistJob(*j) for j in sse])
    return wu.pack_jobs(wtd), np.frombuffer(sse_arr, np.uint8).copy(), len(wtd), luma_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--signal", type=int, default=wu.SDR)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    bd = 10
    n_samples = W * H * 3 // 2
    org = rng.integers(64, 940, n_samples).astype(np.int16)
    cur = np.clip(org + rng.integers(-20, 21, n_samples), 0, 1023).astype(np.int16)
    wtd_jobs, sse_jobs, n, luma_bytes = jobs_for_picture(a.signal)
    ctx = Context(0)
    ctx.set_luma_level_weights(wu.random_table(rng, bd), bd, a.signal, 0.9, wu.random_inv_lut(rng, bd))
    d_org, d_cur = ctx.to_device(org), ctx.to_device(cur)
    d_wj, d_sj = ctx.to_device(wtd_jobs), ctx.to_device(sse_jobs)
    d_w, d_s = ctx.alloc(8 * n), ctx.alloc(8 * n)

    def run_wtd():
        ctx.sse_wtd_batch(d_org.ptr, d_cur.ptr, d_org.ptr, d_wj.ptr, n, d_w.ptr)

    def run_sse():
        ctx.dist_batch(d_org.ptr, d_cur.ptr, d_sj.ptr, n, d_s.ptr)

    def timed(fn):
        ctx.timer_start()
        for _ in range(a.iters):
            fn()
        return ctx.timer_stop_ms() * 1000.0 / a.iters

    for _ in range(3):   # warm-up
        run_wtd()
        run_sse()
    ctx.sync()
    tw, ts = [], []
    for _ in range(a.reps):
        tw.append(timed(run_wtd))
        ts.append(timed(run_sse))
    # both kernels evaluated every job
    w_out, s_out = d_w.to_host(np.uint64), d_s.to_host(np.uint64)
    assert not np.any(w_out == lib.WTD_INVALID_DIST) and np.all(s_out > 0)
    ctx.close()
    sample_bytes = 4 * n_samples * 4          # 4 levels, org + cur int16
    med_w, med_s = float(np.median(tw)), float(np.median(ts))
    res = dict(metric="wtd_bench", picture="1920x1088 4:2:0", levels=[64, 32, 16, 8], jobs=n, signal=a.signal, launches_per_picture=1,
               wtd_us=dict(median=round(med_w, 2), min=round(min(tw), 2), max=round(max(tw), 2)),
               sse_us=dict(median=round(med_s, 2), min=round(min(ts), 2), max=round(max(ts), 2)),
               ratio_wtd_over_sse=round(med_w / med_s, 3),
               wtd_hbm_share=round((sample_bytes + luma_bytes + len(wtd_jobs)) / (med_w * 1e-6) / HBM_PEAK, 3),
               sse_hbm_share=round((sample_bytes + len(sse_jobs)) / (med_s * 1e-6) / HBM_PEAK, 3), reps=a.reps, iters=a.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
