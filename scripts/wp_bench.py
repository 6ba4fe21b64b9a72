"""Times the explicit weighted-prediction kernels against their plain counterparts on the same blocks: every CU of a 64x64 / 32x32 / 16x16 / 8x8 luma
quadtree of one 1920x1088 picture (510 + 2040 + 8160 + 32640 = 43 350 blocks), one launch per batch.
  - vtmhip_wp_dist_batch_dev (xGetSADw / xGetHADsw / xGetSSEw, uni, a non-default weight with an offset, no early exit) against vtmhip_dist_batch_dev
    (xGetSAD / xGetHADs / xGetSSE) per kind;
  - vtmhip_wp_pred_batch_dev (addWeightBi) against vtmhip_add_avg_batch_dev (addAvg) on 14-bit intermediates.
Device events around a run of launches after warm-up; the weighted and the plain kernel alternate, the pair is repeated.

    python scripts/wp_bench.py [--reps 9] [--iters 20]

Prints one JSON line: us per batch (median, min, max over the repetitions) for each pair and the ratio weighted / plain."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import wp_util as wu  # noqa: E402
from vtm_amd import lib  # noqa: E402
from vtm_amd.device import Context  # noqa: E402

W, H, BD = 1920, 1088, 10


def blocks():
    return [(y * W + x, s) for s in (64, 32, 16, 8) for y in range(0, H, s) for x in range(0, W, s)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    org = rng.integers(64, 940, W * H).astype(np.int16)
    cur = np.clip(org + rng.integers(-20, 21, W * H), 0, 1023).astype(np.int16)
    tmp = rng.integers(-4000, 12000, 2 * W * H).astype(np.int16)   # two 14-bit intermediate planes
    bl = blocks()
    n = len(bl)
    wp = wu.derive_uni(45, 12, 5, BD)
    b = wu.derive_bi(45, 12, 20, -3, 5, BD)
    ctx = Context(0)
    d_org, d_cur, d_tmp = ctx.to_device(org), ctx.to_device(cur), ctx.to_device(tmp)
    d_a, d_b = ctx.alloc(8 * n), ctx.alloc(8 * n)
    d_pa, d_pb = ctx.alloc(2 * W * H), ctx.alloc(2 * W * H)
    pairs = {}
    for kind, name in ((lib.DIST_SAD, "sad"), (lib.DIST_SATD, "satd"), (lib.DIST_SSE, "sse")):
        wj = wu.pack_dist_jobs([dict(orgOff=o, curOff=o, orgStride=W, curStride=W, width=s, height=s, kind=kind, bitDepth=BD, isBiPred=0, wp=wp,
                                     maxDist=wu.U64) for o, s in bl])
        pj = (lib.DistJob * n)(*[lib.DistJob(o, o, W, W, s, s, 0, kind) for o, s in bl])
        d_wj, d_pj = ctx.to_device(wj), ctx.to_device(np.frombuffer(pj, np.uint8).copy())
        pairs[name] = (lambda d_wj=d_wj: ctx.wp_dist_batch(d_org.ptr, d_cur.ptr, d_wj.ptr, n, d_a.ptr),
                       lambda d_pj=d_pj: ctx.dist_batch(d_org.ptr, d_cur.ptr, d_pj.ptr, n, d_b.ptr))
    # every CU of the quadtree, each level writing the same picture-sized destination (the ops are per sample)
    wpj = wu.pack_pred_jobs([dict(src0Off=o, src1Off=W * H + o, dstOff=o, src0Stride=W, src1Stride=W, dstStride=W, width=s, height=s, bitDepth=BD,
                                  mode=lib.WP_BI, w0=b[0], w1=b[1], offset=b[2], shift=b[3], round=b[4]) for o, s in bl])
    aj = (lib.PelOpJob * n)(*[lib.PelOpJob(aOff=o, bOff=W * H + o, dstOff=o, aStride=W, bStride=W, dstStride=W, width=s, height=s, bitDepth=BD) for o, s in bl])
    d_wpj, d_aj = ctx.to_device(wpj), ctx.to_device(np.frombuffer(aj, np.uint8).copy())
    pairs["pred"] = (lambda: ctx.wp_pred_batch(d_tmp.ptr, d_tmp.ptr, d_pa.ptr, d_wpj.ptr, n),
                     lambda: ctx.add_avg_batch(d_tmp.ptr, d_tmp.ptr, d_pb.ptr, d_aj.ptr, n))

    def timed(fn):
        ctx.timer_start()
        for _ in range(a.iters):
            fn()
        return ctx.timer_stop_ms() * 1000.0 / a.iters

    res = dict(metric="wp_bench", picture="1920x1088 luma", levels=[64, 32, 16, 8], jobs=n, bitDepth=BD, reps=a.reps, iters=a.iters)
    for name, (fw, fp) in pairs.items():
        for _ in range(3):   # warm-up
            fw()
            fp()
        ctx.sync()
        tw, tp = [], []
        for _ in range(a.reps):
            tw.append(timed(fw))
            tp.append(timed(fp))
        if name != "pred":   # every job evaluated
            assert not np.any(d_a.to_host(np.uint64) == lib.WP_INVALID_DIST) and np.all(d_b.to_host(np.uint64) > 0)
        res[name] = dict(weighted_us=dict(median=round(float(np.median(tw)), 2), min=round(min(tw), 2), max=round(max(tw), 2)),
                         plain_us=dict(median=round(float(np.median(tp)), 2), min=round(min(tp), 2), max=round(max(tp), 2)),
                         ratio=round(float(np.median(tw) / np.median(tp)), 3))
    # spot check: the weighted SAD batch against the restatement on a few blocks
    pairs["sad"][0]()
    out = d_a.to_host(np.uint64)
    for i in range(0, n, n // 7):
        o, s = bl[i]
        ob = org.reshape(H, W)[o // W:o // W + s, o % W:o % W + s]
        cb = cur.reshape(H, W)[o // W:o // W + s, o % W:o % W + s]
        assert int(out[i]) == wu.sad_w(ob, cb, wp, BD, 0), i
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
