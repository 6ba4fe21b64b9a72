"""Times the joint Cb-Cr chain (vtmhip_jccr_chain_batch_dev) against the two plain chains (vtmhip_tu_chain_batch_dev on Cb, then on Cr) of the same TUs:
the 4:2:0 chroma TU pairs of a 64 / 32 / 16 / 8 luma quadtree of one 1920x1088 picture -- 510 + 2040 + 8160 + 32640 pairs of 32x32 / 16x16 / 8x8 / 4x4 --
each level one uniform launch (the plain side: one uniform launch of 2 n jobs, Cb then Cr).
Device events around a run of calls after warm-up; joint and plain alternate, the pair is repeated.  The joint call reads its job table back and checks it
on the host before it launches, so besides the call time the kernels' own time is reported (vtmhip_kernel_timing, a run of its own).

    python scripts/jccr_bench.py [--reps 9] [--iters 20]

Prints one JSON line: us per level (median, min, max over the repetitions) for both sides and the ratio joint / plain."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import jccr_util as ju  # noqa: E402
from vtm_amd import lib  # noqa: E402
from vtm_amd.device import Context  # noqa: E402

CW, CH, BD, QP = 960, 544, 10, 32 + 12
MASKS = [(3, 0), (2, 0), (1, 0), (3, 1), (2, 1), (1, 1)]   # (cbfMask, signFlag): all six joint modes in turn


def stats(v):
    return dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    cb = rng.integers(-60, 61, (CH, CW)).astype(np.int16)
    cr = np.clip(cb.astype(np.int32) * 3 // 4 + rng.integers(-15, 16, (CH, CW)), -1023, 1023).astype(np.int16)   # correlated, as where the joint mode is tried
    ctx = Context(0)
    d_resi = ctx.to_device(np.concatenate([cb.reshape(-1), cr.reshape(-1)]))
    d_lv = ctx.alloc(4 * 2 * CW * CH)
    res = dict(metric="jccr_bench", picture="1920x1088 4:2:0 chroma", bitDepth=BD, qp=QP - 12, reps=a.reps, iters=a.iters, levels={})
    for s in (32, 16, 8, 4):
        pos = [(y, x) for y in range(0, CH, s) for x in range(0, CW, s)]
        n = len(pos)
        jj, tj = (lib.JccrJob * n)(), (lib.TuJob * (2 * n))()
        for k, (y, x) in enumerate(pos):
            j = jj[k]
            j.cbOff, j.crOff, j.outOff, j.resiStride, j.width, j.height = y * CW + x, CW * CH + y * CW + x, k * s * s, CW, s, s
            j.qpPer, j.qpRem, j.typeHor, j.bitDepth, j.isIRAP = QP // 6, QP % 6, lib.DCT2, BD, 0
            j.cbfMask, j.signFlag = MASKS[k % 6]
            for c in range(2):
                t = tj[c * n + k]
                t.resiOff, t.outOff, t.resiStride, t.width, t.height = c * CW * CH + y * CW + x, (c * n + k) * s * s, CW, s, s
                t.qpPer, t.qpRem, t.typeHor, t.typeVer, t.bitDepth, t.isIRAP = QP // 6, QP % 6, lib.DCT2, lib.DCT2, BD, 0
        d_jj, d_tj = ctx.to_device(np.frombuffer(jj, np.uint8).copy()), ctx.to_device(np.frombuffer(tj, np.uint8).copy())
        d_rj, d_rt = ctx.alloc(C.sizeof(lib.JccrResult) * n), ctx.alloc(C.sizeof(lib.TuResult) * 2 * n)

        def joint():
            ctx.jccr_chain_batch(d_resi.ptr, d_jj.ptr, n, s, s, d_rj.ptr, d_lv.ptr, None, None, uniform=True)

        def plain():
            ctx.tu_chain_batch(d_resi.ptr, d_tj.ptr, 2 * n, s, s, d_rt.ptr, d_lv.ptr, None, uniform=True)

        def timed(fn):
            ctx.timer_start()
            for _ in range(a.iters):
                fn()
            return ctx.timer_stop_ms() * 1000.0 / a.iters

        for _ in range(3):   # warm-up
            joint()
            plain()
        ctx.sync()
        tjn, tpl = [], []
        for _ in range(a.reps):
            tjn.append(timed(joint))
            tpl.append(timed(plain))
        # the kernels alone
        ctx.kernel_timing(True)
        for _ in range(a.iters):
            joint()
            plain()
        kname = "lane" if s == 4 else "uni"
        kj, nj = ctx.kernel_timing_read("jccr_chain_%s_kernel" % kname)
        kp, npl = ctx.kernel_timing_read("tu_chain_%s_kernel" % kname)
        ctx.kernel_timing(False)
        assert nj == a.iters and npl == a.iters
        # spot check: a few pairs against the expectation composed from the restatement and the oracle
        got = (lib.JccrResult * n).from_buffer_copy(d_rj.to_host(np.uint8).tobytes())
        for k in range(0, n, max(1, n // 5)):
            y, x = pos[k]
            e = ju.chain_expect(cb[y:y + s, x:x + s], cr[y:y + s, x:x + s], jj[k].cbfMask, jj[k].signFlag, BD, QP // 6, QP % 6, 0, False)
            assert (got[k].sseCb, got[k].sseCr, got[k].fwdDist, got[k].sumAbs, got[k].absSum) == (e["sseCb"], e["sseCr"], e["fwdDist"], e["sumAbs"], e["absSum"]), (s, k)
        res["levels"]["%dx%d" % (s, s)] = dict(pairs=n, coded=sum(r.absSum > 0 for r in got), joint_us=stats(tjn), plain_pair_us=stats(tpl),
                                               ratio=round(float(np.median(tjn) / np.median(tpl)), 3), joint_kernel_us=round(kj * 1000.0 / nj, 2),
                                               plain_kernel_us=round(kp * 1000.0 / npl, 2), kernel_ratio=round(kj / kp, 3))
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
