"""Times the SBT entries on a seeded 4K-picture-sized job set: the CUs of bench.py's default (quadtree) partition that may use SBT -- the 64 / 32 / 16 / 8 levels
of one 3840x2176 4:2:0 picture, 2040 + 8160 + 32640 + 130560 CUs, each level covering the picture -- with four candidates per CU (two half and two quarter
modes, drawn per CU; the four half modes for 8x8).

  (a) vtmhip_sbt_est_batch_dev: one launch per level, every CU with chroma.
  (b) vtmhip_sbt_chain_batch_dev against vtmhip_tu_chain_batch_dev (uniformSize 0) on the identical sub-TU job list prepared on the host by
      vtmhip_sbt_make_tu_jobs, in the same process, both writing levels and reconstruction.  The difference is the cost of the table read-back, the
      expansion and the finish kernel.

    python scripts/sbt_bench.py [--reps 5] [--iters 5]

Clock: device events on the context's stream around `iters` back-to-back calls (vtmhip_timer_start / stop), after three warm-up rounds of every side; the two
sides of (b) alternate, the pair is repeated `reps` times; median, min and max over the repetitions.  Both chain entries synchronise the stream once per call
(the SBT entry to read its table back, the plain chain to read the bucket counts), so the event time includes those waits.  A few candidates per level are
checked against the restatement of tests/sbt_util.py.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import sbt_util as su  # noqa: E402
from vtm_amd import device, lib  # noqa: E402
from vtm_amd.device import Context  # noqa: E402

LW, LH, BD, QP, QPC = 3840, 2176, 10, 32, 33
CW, CH = LW // 2, LH // 2
OFF = (0, LW * LH, LW * LH + CW * CH)   # Y, Cb, Cr planes inside one buffer
STRIDE = (LW, CW, CW)


def stats(v):
    return dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--levels", type=str, default="64,32,16,8")
    a = ap.parse_args()
    rng = np.random.default_rng(4)
    planes = [rng.integers(-60, 61, (LH, LW)).astype(np.int16), rng.integers(-25, 26, (CH, CW)).astype(np.int16), rng.integers(-25, 26, (CH, CW)).astype(np.int16)]
    resi = np.concatenate([p.reshape(-1) for p in planes])
    org = np.clip(512 + resi, 0, 1023).astype(np.int16)
    pred = np.full_like(org, 512)
    ctx = Context(0)
    d_resi, d_org, d_pred = ctx.to_device(resi), ctx.to_device(org), ctx.to_device(pred)
    slots = 4 * (LW * LH + 2 * CW * CH)      # CU-shaped output blocks of four candidates per CU
    d_lv, d_rec = ctx.alloc(4 * slots), ctx.alloc(2 * slots)
    res = dict(metric="sbt_bench", picture="%dx%d 4:2:0" % (LW, LH), bitDepth=BD, qp=QP, reps=a.reps, iters=a.iters, clock="device events around iters calls, 3 warm-up rounds",
               levels={})
    per, rem = su.qp_of(QP, BD)
    perc, remc = su.qp_of(QPC, BD)

    def timed(fn):
        ctx.timer_start()
        for _ in range(a.iters):
            fn()
        return ctx.timer_stop_ms() * 1000.0 / a.iters

    def alternate(f, g):
        for _ in range(3):
            f()
            g()
        ctx.sync()
        tf, tg = [], []
        for _ in range(a.reps):
            tf.append(timed(f))
            tg.append(timed(g))
        return tf, tg

    tot = dict(est=0.0, sbt=0.0, plain=0.0)
    for s in [int(v) for v in a.levels.split(",")]:
        ys, xs = np.meshgrid(np.arange(0, LH, s), np.arange(0, LW, s), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        ncu = ys.size
        # ---- (a) the estimator
        ej = np.zeros(ncu, np.dtype(lib.SbtEstJob))
        for c in range(3):
            sh = 0 if c == 0 else 1
            ej["orgOff"][:, c] = ej["predOff"][:, c] = OFF[c] + (ys >> sh) * STRIDE[c] + (xs >> sh)
            ej["orgStride"][:, c] = ej["predStride"][:, c] = STRIDE[c]
        ej["width"], ej["height"], ej["bitDepth"], ej["sbtAllowed"], ej["chromaWeight"], ej["distScale"] = s, s, BD, su.sbt_allowed(s, s), 0.8137, 1.0 / 57.3
        d_ej, d_er = ctx.to_device(ej.view(np.uint8)), ctx.alloc(C.sizeof(lib.SbtEstResult) * ncu)

        def est():
            ctx.sbt_est_batch(d_org.ptr, d_pred.ptr, d_ej.ptr, ncu, s, s, d_er.ptr)

        t_est, _ = alternate(est, est)
        er = (lib.SbtEstResult * ncu).from_buffer_copy(d_er.to_host(np.uint8).tobytes())
        for k in range(0, ncu, max(1, ncu // 4)):
            y, x = int(ys[k]), int(xs[k])
            part = [su.part_sums(planes[c][y >> (c > 0):(y + s) >> (c > 0), x >> (c > 0):(x + s) >> (c > 0)], np.zeros((s >> (c > 0), s >> (c > 0)), np.int16),
                                 su.num_part(s), su.num_part(s), BD) for c in range(3)]   # org - pred is the residual plane
            e = su.combine(part, s, s, su.sbt_allowed(s, s), 0.8137, 1.0 / 57.3)
            assert (list(er[k].est), list(er[k].rdoOrder), er[k].skipAll) == (e["est"], e["order"], e["skipAll"]), (s, k)
        # ---- (b) the candidate chain: four candidates per CU
        n = 4 * ncu
        if s >= 16:
            modes = np.concatenate([np.argsort(rng.random((ncu, 4)), axis=1)[:, :2], 4 + np.argsort(rng.random((ncu, 4)), axis=1)[:, :2]], axis=1)
        else:
            modes = np.tile(np.arange(4), (ncu, 1))
        sj = np.zeros(n, np.dtype(lib.SbtJob))
        cu = np.repeat(np.arange(ncu), 4)
        m = modes.reshape(-1)
        out = 0
        for c in range(3):
            sh = 0 if c == 0 else 1
            sj["resiOff"][:, c] = OFF[c] + (ys[cu] >> sh) * STRIDE[c] + (xs[cu] >> sh)
            sj["resiStride"][:, c] = STRIDE[c]
            sj["outOff"][:, c] = out + np.arange(n, dtype=np.int64) * ((s >> sh) ** 2)
            out += n * ((s >> sh) ** 2)
            sj["qpPer"][:, c], sj["qpRem"][:, c] = (per, rem) if c == 0 else (perc, remc)
        assert out <= slots
        sj["width"], sj["height"], sj["sbtIdx"], sj["sbtPos"], sj["bitDepth"], sj["isIRAP"] = s, s, 1 + m // 2, m % 2, BD, 0
        jobs = (lib.SbtJob * n).from_buffer(sj)
        tu, tu_idx = device.sbt_make_tu_jobs(jobs)
        ntu = len(tu)
        tua = np.frombuffer(tu, np.dtype(lib.TuJob))
        mw, mh = int(tua["width"].max()), int(tua["height"].max())
        d_sj, d_sr = ctx.to_device(sj.view(np.uint8)), ctx.alloc(C.sizeof(lib.SbtResult) * n)
        d_tu, d_tr = ctx.to_device(np.frombuffer(tu, np.uint8).copy()), ctx.alloc(C.sizeof(lib.TuResult) * ntu)

        def sbt():
            ctx.sbt_chain_batch(d_resi.ptr, d_sj.ptr, n, d_sr.ptr, d_lv.ptr, d_rec.ptr)

        def plain():
            ctx.tu_chain_batch(d_resi.ptr, d_tu.ptr, ntu, mw, mh, d_tr.ptr, d_lv.ptr, d_rec.ptr)

        t_sbt, t_plain = alternate(sbt, plain)
        plain()
        tr = (lib.TuResult * ntu).from_buffer_copy(d_tr.to_host(np.uint8).tobytes())
        sbt()
        sr = (lib.SbtResult * n).from_buffer_copy(d_sr.to_host(np.uint8).tobytes())
        for k in range(0, n, max(1, n // 6)):
            y, x, mode = int(ys[cu[k]]), int(xs[cu[k]]), int(m[k])
            for c in range(3):
                sh = c > 0
                r = planes[c][y >> sh:(y + s) >> sh, x >> sh:(x + s) >> sh]
                e = su.chain_expect(r, su.idx_from_mode(mode), su.pos_from_mode(mode), c == 0, BD, per if c == 0 else perc, rem if c == 0 else remc, 0)
                assert (sr[k].sseCoded[c], sr[k].sseZero[c], sr[k].absSum[c]) == (e["sseCoded"], e["sseZero"], e["absSum"]), (s, k, c)
                t = tr[int(tu_idx[k, c])]
                assert (t.sse, t.absSum) == (e["sseCoded"], e["absSum"]), (s, k, c)
        coded = sum(1 for k in range(0, n, 97) if sr[k].absSum[0] > 0) / len(range(0, n, 97))
        res["levels"]["%dx%d" % (s, s)] = dict(cus=int(ncu), candidates=int(n), sub_tus=int(ntu), est_us=stats(t_est), sbt_chain_us=stats(t_sbt), tu_chain_us=stats(t_plain),
                                               ratio=round(float(np.median(t_sbt) / np.median(t_plain)), 3), luma_coded_share=round(coded, 3))
        tot["est"] += float(np.median(t_est))
        tot["sbt"] += float(np.median(t_sbt))
        tot["plain"] += float(np.median(t_plain))
        for d in (d_ej, d_er, d_sj, d_sr, d_tu, d_tr):
            d.free()
    res["picture_total_us"] = dict(estimator=round(tot["est"], 1), sbt_chain=round(tot["sbt"], 1), tu_chain=round(tot["plain"], 1), ratio=round(tot["sbt"] / tot["plain"], 3),
                                   expansion_plus_finish=round(tot["sbt"] - tot["plain"], 1))
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
