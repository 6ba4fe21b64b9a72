"""Times the GEO merge estimation of B CUs of one shape, six candidates each, 10 bit, SATD:

  (f) vtmhip_geo_cand_satd_batch_dev: one fused kernel per batch, nothing read back;
  (c) the composition the other entries allow: vtmhip_mc_batch_dev (bi = 1: the 14-bit blocks), vtmhip_weightedGeoBlk_batch_dev over a plane of eights (a weight
      of 8 on both sources is roundToOutputBitdepth: the device has no rounding entry of its own), vtmhip_dist_batch_dev (the whole-block SADs) and
      vtmhip_masked_sad_batch_dev over 384 jobs per CU with the uploaded mask planes; the read-back of both SAD tables; the costs, the filter and the ordered list on
      the host (numpy, vectorised over the batch: one stable sort per CU); the upload of the blend and distortion jobs; vtmhip_weightedGeoBlk_batch_dev with the
      uploaded weight planes and vtmhip_dist_batch_dev.

    python scripts/geo_cand_bench.py [--blocks 2048] [--reps 5] [--window 0.5] [--out profiles/geo_cand_ab.txt]

Planes and the static job tables are resident.  A measurement is a window of at least `window` seconds of runs of one route, ended by a stream synchronisation, under
the host's clock and -- for the fused route -- between two device events, divided by the number of runs; the runs per window come from one short window of each route
after two warm-up rounds of both; the routes alternate, `reps` times; median, min and max per batch in microseconds, spread = ( max - min ) / median.  Behind each
composition window four fused runs are timed between device events as well: the short window in which the fused kernel runs right behind other kernels.
The composition's parts (device stage one, read-back, host list, upload, device stage two) are timed inside it with a synchronisation after each.  The two routes'
lists and distortions are compared in full before timing.  Prints one JSON line and, with --out, a table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import geo_util as gu  # noqa: E402
from vtm_amd import lib  # noqa: E402
from vtm_amd.device import Context  # noqa: E402

BD, MARGIN, SLACK, NC, LAMBDA = 10, 160, 2048, 6, 20.37
PIC_W, PIC_H = 4096, 2048
REF_STRIDE = PIC_W + 2 * MARGIN
PLANE = (PIC_H + 2 * MARGIN) * REF_STRIDE
M = gu.M


def stats(v):
    return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1), spread=round((max(v) - min(v)) / float(np.median(v)), 3))


def ref_off(l, x, y):
    return SLACK + l * PLANE + (MARGIN + y) * REF_STRIDE + MARGIN + x


def table(struct, n, **cols):
    t = np.zeros(n, np.dtype(struct))
    for k, v in cols.items():
        t[k] = v
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--sizes", type=str, default="8x8,16x16,32x32,64x64")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    rng = np.random.default_rng(21)
    ctx = Context(0)
    # a textured picture; list 0 and list 1 are noisy copies of it, the original a third one: candidates resemble the original, as merge candidates do
    yy, xx = np.mgrid[0:PIC_H + 2 * MARGIN, 0:REF_STRIDE]
    base = (np.sin(xx / 9.0) + np.cos(yy / 6.0) + np.sin((xx + yy) / 23.0) + 3.0) / 6.0 * 900.0
    planes = [np.clip(base + rng.integers(-40, 41, base.shape), 0, 1023).astype(np.int16).reshape(-1) for _ in range(2)]
    org = np.clip(base[MARGIN:MARGIN + PIC_H, MARGIN:MARGIN + PIC_W] + rng.integers(-25, 26, (PIC_H, PIC_W)), 0, 1023).astype(np.int16)
    refs = np.concatenate([np.zeros(SLACK, np.int16)] + planes + [np.zeros(SLACK, np.int16)])
    d_org, d_ref = ctx.to_device(org), ctx.to_device(refs)
    wplanes, mplanes = gu.weight_planes(), gu.mask_planes()
    d_wp, d_mp = ctx.to_device(wplanes.reshape(-1)), ctx.to_device(mplanes.reshape(-1))
    pairs = np.array(gu.PAIRS)
    res = dict(metric="geo_cand_bench", blocks=a.blocks, bitDepth=BD, candidates_per_cu=NC, sqrtLambda=LAMBDA, reps=a.reps, window_s=a.window,
               clock="host clock, and device events, around a window of runs + stream sync, per batch (us)", sizes={})
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        per_row, area = PIC_W // w, w * h
        B = min(a.blocks, per_row * (PIC_H // h))
        bx, by = (np.arange(B) % per_row) * w, (np.arange(B) // per_row) * h
        org_off = by * PIC_W + bx
        mv = rng.integers(-40, 41, (B, NC, 2))
        lst = (np.arange(B)[:, None] + np.arange(NC)[None, :]) & 1
        roff = SLACK + lst * PLANE + (MARGIN + by[:, None]) * REF_STRIDE + MARGIN + bx[:, None]
        # ---- the fused route's table ----
        jobs = (lib.GeoJob * B)()
        for b in range(B):
            jobs[b] = gu.geo_job(w, h, BD, NC, LAMBDA, org_off=int(org_off[b]), org_stride=PIC_W,
                                 cands=[(int(roff[b, c]), REF_STRIDE, int(mv[b, c, 0]), int(mv[b, c, 1]), -1) for c in range(NC)])
        d_jobs = ctx.to_device(np.frombuffer(jobs, np.uint8).copy())
        d_res = ctx.alloc(B * lib.C.sizeof(lib.GeoResult))
        # ---- the composition's static tables: plane14 [B][6][area], rounded behind it, an all-8 weight block, the blends behind that ----
        n6 = B * NC
        blk = (np.arange(n6) * area).astype(np.int64)
        mc = table(lib.McJob, n6, refOff=roff.reshape(-1), dstOff=blk, refStride=REF_STRIDE, dstStride=w, width=w, height=h, mvHor=mv[:, :, 0].reshape(-1),
                   mvVer=mv[:, :, 1].reshape(-1), bi=1, bitDepth=BD)
        rnd = table(lib.GeoBlendJob, n6, src0Off=blk, src1Off=blk, dstOff=blk, weightOff=0, src0Stride=w, src1Stride=w, dstStride=w, weightStride=w, width=w, height=h, stepX=1)
        whole = table(lib.DistJob, n6, orgOff=np.repeat(org_off, NC), curOff=blk, orgStride=PIC_W, curStride=w, width=w, height=h, kind=lib.DIST_SAD)
        sw = np.array([gu.sad_walk(s, w, h) for s in range(64)])          # plane, first, maskStride, stepX, maskStride2
        bwk = np.array([gu.blend_walk(s, w, h, 0) for s in range(64)])    # plane, first, stepX, row step
        nm = B * 64 * NC
        msad = table(lib.MaskedSadJob, nm, orgOff=np.repeat(org_off, 64 * NC), curOff=np.repeat(blk.reshape(B, 1, NC), 64, 1).reshape(-1),
                     maskOff=np.tile(np.repeat(sw[:, 0] * M * M + sw[:, 1], NC), B), orgStride=PIC_W, curStride=w, maskStride=np.tile(np.repeat(sw[:, 2], NC), B),
                     maskStride2=np.tile(np.repeat(sw[:, 4], NC), B), width=w, height=h, stepX=np.tile(np.repeat(sw[:, 3], NC), B))
        d_mc, d_rnd, d_whole, d_msad = (ctx.to_device(t.view(np.uint8)) for t in (mc, rnd, whole, msad))
        d_p14, d_round, d_eight = ctx.alloc(2 * n6 * area), ctx.alloc(2 * n6 * area), ctx.to_device(np.full(area, 8, np.int16))
        d_blend = ctx.alloc(2 * B * 60 * area)
        d_sw, d_sl, d_dist = ctx.alloc(8 * n6), ctx.alloc(8 * nm), ctx.alloc(8 * B * 60)
        d_bj, d_dj = ctx.alloc(B * 60 * lib.C.sizeof(lib.GeoBlendJob)), ctx.alloc(B * 60 * lib.C.sizeof(lib.DistJob))
        c0s, c1s = pairs[:, 0], pairs[:, 1]
        bits = (np.arange(NC) + 1).astype(np.float64) * np.float64(LAMBDA)
        parts = dict(device_sads=[], read_back=[], host_list=[], upload=[], device_blend_dist=[])
        last = {}

        def route_f():
            ctx.geo_cand_satd_batch(d_ref.ptr, d_org.ptr, None, d_jobs.ptr, B, w, h, d_res.ptr)

        def route_c(record=None):
            t0 = time.perf_counter()
            ctx.mc_batch(d_ref.ptr, d_p14.ptr, d_mc.ptr, n6, w, h)
            ctx.weightedGeoBlk_batch(d_p14.ptr, d_round.ptr, d_eight.ptr, d_rnd.ptr, n6, BD, (0, 1023))
            ctx.dist_batch(d_org.ptr, d_round.ptr, d_whole.ptr, n6, d_sw.ptr)
            ctx.masked_sad_batch(d_org.ptr, d_round.ptr, d_mp.ptr, d_msad.ptr, nm, d_sl.ptr)
            ctx.sync()
            t1 = time.perf_counter()
            sad_w = d_sw.to_host(np.uint64).reshape(B, NC)
            sad_l = d_sl.to_host(np.uint64).reshape(B, 64, NC)
            t2 = time.perf_counter()
            # the first pass on the host, vectorised over the batch; a stable sort of ( split, pair ) order is the list order
            first_min = np.argmin(sad_w, 1)
            best = sad_w[np.arange(B), first_min].astype(np.float64) + bits[first_min]
            cost0 = sad_l.astype(np.float64) + bits
            cost1 = (sad_w[:, None, :] - sad_l).astype(np.float64) + bits
            t = cost0[:, :, c0s] + cost1[:, :, c1s]                                   # [B][64][30]
            keep = ~(t > best[:, None, None])
            cost = np.where(keep, t + np.float64(6) * np.float64(LAMBDA), np.inf).reshape(B, 1920)
            order = np.argsort(cost, 1, kind="stable")[:, :60]
            listed = np.take_along_axis(cost, order, 1)
            valid = np.isfinite(listed)
            split, pair = order // 30, order % 30
            cb = np.arange(B)[:, None]
            s0 = ((cb * NC + c0s[pair]) * area)[valid]
            s1 = ((cb * NC + c1s[pair]) * area)[valid]
            nb = int(valid.sum())
            dst = (np.arange(nb) * area).astype(np.int64)
            sp = split[valid]
            bj = table(lib.GeoBlendJob, nb, src0Off=s0, src1Off=s1, dstOff=dst, weightOff=bwk[sp, 0] * M * M + bwk[sp, 1], src0Stride=w, src1Stride=w, dstStride=w,
                       weightStride=bwk[sp, 3], width=w, height=h, stepX=bwk[sp, 2])
            dj = table(lib.DistJob, nb, orgOff=np.broadcast_to(org_off[:, None], valid.shape)[valid], curOff=dst, orgStride=PIC_W, curStride=w, width=w, height=h,
                       kind=lib.DIST_SATD)
            t3 = time.perf_counter()
            if nb:
                d_bj.upload(bj.view(np.uint8))
                d_dj.upload(dj.view(np.uint8))
                ctx.sync()
            t4 = time.perf_counter()
            if nb:
                ctx.weightedGeoBlk_batch(d_p14.ptr, d_blend.ptr, d_wp.ptr, d_bj.ptr, nb, BD, (0, 1023))
                ctx.dist_batch(d_org.ptr, d_blend.ptr, d_dj.ptr, nb, d_dist.ptr)
            ctx.sync()
            t5 = time.perf_counter()
            if record is not None:
                for k, v in zip(("device_sads", "read_back", "host_list", "upload", "device_blend_dist"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                    record[k].append(v * 1e6)
            last.update(valid=valid, split=split, pair=pair, cost=listed, nb=nb, passed=keep.reshape(B, -1).sum(1))

        def wall(fn, inner, **kw):
            """-> (host clock, device events): microseconds per run of `inner` runs ended by a stream synchronisation"""
            ctx.sync()
            t = time.perf_counter()
            ctx.timer_start()
            for _ in range(inner):
                fn(**kw)
            ev = ctx.timer_stop_ms()      # records the stop event behind the runs and waits for it
            ctx.sync()
            return (time.perf_counter() - t) * 1e6 / inner, ev * 1e3 / inner

        for _ in range(2):
            route_f()
            route_c()
        ctx.sync()
        # the two routes agree: the list members, their costs and the distortions
        got = np.frombuffer(d_res.to_host(np.uint8).tobytes(), np.dtype(lib.GeoResult))
        dist_c = d_dist.to_host(np.uint64)[:last["nb"]]
        v = last["valid"]
        assert np.array_equal(got["numPassed"], last["passed"]) and np.array_equal(got["numTested"], v.sum(1)), "the two routes disagree at %s" % size
        assert np.array_equal(got["combo"]["splitDir"][v], last["split"][v]) and np.array_equal(got["combo"]["cost"][v], last["cost"][v])
        assert np.array_equal(got["combo"]["cand0"][v], c0s[last["pair"]][v]) and np.array_equal(got["combo"]["cand1"][v], c1s[last["pair"]][v])
        assert np.array_equal(got["combo"]["dist"][v], dist_c), "the two routes' distortions disagree at %s" % size
        # windows of at least a.window seconds: the number of runs per window comes from one short window of each route
        inner_f = max(4, int(np.ceil(a.window * 1e6 / wall(route_f, 4)[0])))
        inner_c = max(1, int(np.ceil(a.window * 1e6 / wall(route_c, 1)[0])))
        t = dict(f=[], f_ev=[], c=[], f_short=[])
        for _ in range(a.reps):
            host, ev = wall(route_f, inner_f)
            t["f"].append(host)
            t["f_ev"].append(ev)
            t["c"].append(wall(route_c, inner_c, record=parts)[0])
            t["f_short"].append(wall(route_f, 4)[1])      # four fused runs right behind a composition run: what a short window sees there
        f, fe, fs, c = stats(t["f"]), stats(t["f_ev"]), stats(t["f_short"]), stats(t["c"])
        dev = float(np.median(parts["device_sads"]) + np.median(parts["device_blend_dist"]))
        copies = float(np.median(parts["read_back"]) + np.median(parts["upload"]))
        res["sizes"][size] = dict(cus=B, lanes_per_job=ctx.L.vtmhip_geo_lanes_per_job(w, h), mean_passed=round(float(last["passed"].mean()), 1),
                                  mean_tested=round(float(v.sum(1).mean()), 1), runs_per_window=dict(fused=inner_f, composition=inner_c), fused_us=f, fused_device_events_us=fe,
                                  fused_four_runs_behind_composition_device_events_us=fs, composition_us=c, fused_us_per_cu=round(fe["median"] / B, 3),
                                  composition_parts_us={k: round(float(np.median(x)), 1) for k, x in parts.items()},
                                  composition_device_parts_over_fused=round(dev / fe["median"], 2),
                                  composition_device_parts_and_copies_over_fused=round((dev + copies) / fe["median"], 2), routes_equal=True)
        for d in (d_jobs, d_res, d_mc, d_rnd, d_whole, d_msad, d_p14, d_round, d_eight, d_blend, d_sw, d_sl, d_dist, d_bj, d_dj):
            d.free()
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("GEO merge estimation, %d CUs per batch, 6 candidates, 10 bit, SATD, sqrtLambda %.2f; microseconds per batch, median of %d windows (min .. max)\n"
                     % (a.blocks, LAMBDA, a.reps))
            fh.write("a window is at least %.2f s of runs of one route ended by a stream synchronisation; the routes alternate\n" % a.window)
            fh.write("fused = vtmhip_geo_cand_satd_batch_dev (host clock; device events; four runs right behind a composition run, device events)\n")
            fh.write("composition = dev1: mc + round + SADs + masked SADs | back: read-back | host: the list in numpy | up: upload | dev2: blend + dist\n\n")
            fh.write("%-6s %5s %6s %6s %11s  %-26s %-26s %-28s %-30s %-34s %s\n" % ("shape", "CUs", "passed", "tested", "runs/window", "fused, host clock", "fused, device events",
                                                                               "fused, 4 runs behind (c)", "composition", "dev1 / back / host / up / dev2", "(dev1+dev2)/f  (+copies)/f"))
            cell = lambda x: "%.1f (%.1f .. %.1f)" % (x["median"], x["min"], x["max"])      # noqa: E731
            for size, e in res["sizes"].items():
                p = e["composition_parts_us"]
                fh.write("%-6s %5d %6.1f %6.1f %5d /%4d  %-26s %-26s %-28s %-30s %-34s %.2f  %.2f\n"
                         % (size, e["cus"], e["mean_passed"], e["mean_tested"], e["runs_per_window"]["fused"], e["runs_per_window"]["composition"], cell(e["fused_us"]),
                            cell(e["fused_device_events_us"]), cell(e["fused_four_runs_behind_composition_device_events_us"]), cell(e["composition_us"]),
                            "%.0f / %.0f / %.0f / %.0f / %.0f" % (p["device_sads"], p["read_back"], p["host_list"], p["upload"], p["device_blend_dist"]),
                            e["composition_device_parts_over_fused"], e["composition_device_parts_and_copies_over_fused"]))


if __name__ == "__main__":
    main()
