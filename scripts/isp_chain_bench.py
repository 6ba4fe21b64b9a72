"""Times the ISP candidates of one intra level -- B square CUs x 3 modes (DC, horizontal, vertical) x 2 split directions; CUs 8 .. 64, 10 bit, base QP 32:

  (c) vtmhip_isp_chain_batch_dev: one call, every sub-partition of a candidate in one kernel, plus the download of its result records;
  (a) the route before that entry, where it exists (sub-partitions with both sides >= 4, so 16x16 and up): four rounds of vtmhip_intra_pred_batch_dev on
      re-uploaded lines -> vtmhip_subtract_batch_dev -> vtmhip_tu_chain_batch_dev -> download -> the lines of the next round and the clipped reconstruction in numpy.
      (The three modes are those for which the plain prediction of a sub-partition as a block of its own is the ISP prediction: no wide-angle shift, no filter, and
      reads inside the first W + 1 / H + 1 samples of the lines.)

    python scripts/isp_chain_bench.py [--blocks 256] [--reps 7]

Both routes start with the upload of the CUs' lines and end with their results on the host; block and job tables are resident.  Clock: the host's, around work that
ends in a stream synchronisation, after two warm-up rounds of every route; the routes alternate, `reps` times; median, min and max.  Device time of (c): events on the
stream around the call (they span the read-back of the tables and their check on the host, during which the device idles) and, from vtmhip_kernel_timing in a pass
of its own, the kernel alone; their difference is the read-back pause.  Every output of the two routes -- predictions, levels, reconstructions, the three sums per
sub-partition -- is compared in full.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vtm_amd import lib  # noqa: E402
from vtm_amd.device import Context, struct_array_to_numpy as s2n  # noqa: E402
from vtm_amd.lib import IntraBlock, IntraJob, IspGeom, IspJob, PelOpJob, TuJob  # noqa: E402

BD, QP = 10, 32
STRIDE = 4096
MODES = (1, 18, 50)
RESULT = np.dtype([("sse", "<u8", 4), ("absSum", "<i4", 4), ("sumAbs", "<i4", 4), ("numParts", "<i4"), ("reserved", "<i4")])
TU_RESULT = np.dtype([("sse", "<u8"), ("sumAbs", "<i4"), ("absSum", "<i4")])


def stats(v):
    return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=str, default="8,16,32,64")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    L = lib.load()
    ctx = Context(0)
    B = a.blocks
    per, rem = divmod(QP + 6 * (BD - 8), 6)
    res = dict(metric="isp_chain_bench", blocks=B, bitDepth=BD, qp=QP, modes=list(MODES), reps=a.reps,
               clock="host clock around calls + stream sync (us); *_dev_us: device events; kernel_us: vtmhip_kernel_timing", sizes={})
    for s in [int(v) for v in a.sizes.split(",")]:
        area, per_row, mx = s * s, STRIDE // s, (1 << BD) - 1
        plane = rng.integers(0, 1 << BD, (((B + per_row - 1) // per_row) * s, STRIDE)).astype(np.int16)
        line_len = 4 * s + 2
        lines = rng.integers(0, 1 << BD, B * line_len).astype(np.int16)
        lines.reshape(B, line_len)[:, 2 * s + 1] = lines.reshape(B, line_len)[:, 0]
        org_off = np.array([(b // per_row) * s * STRIDE + (b % per_row) * s for b in range(B)])
        cands = [(b, m, sp) for b in range(B) for m in MODES for sp in (1, 2)]
        n = len(cands)
        blk_arr, job_arr = (IntraBlock * B)(), (IspJob * n)()
        for b in range(B):
            blk_arr[b] = IntraBlock(b * line_len, int(org_off[b]), STRIDE, s, s, BD, 0)
        for k, (b, m, sp) in enumerate(cands):
            job_arr[k] = IspJob(k * area, k * area, b, per, rem, m, sp, 1, 0)
        d_org, d_lines, d_blk, d_job = (ctx.to_device(v) for v in (plane, lines, s2n(blk_arr), s2n(job_arr)))
        d_pred, d_lev, d_rec, d_res = (ctx.alloc(v) for v in (2 * n * area, 4 * n * area, 2 * n * area, RESULT.itemsize * n))
        out = {}

        def c_call():
            ctx.isp_chain_batch(d_lines.ptr, d_org.ptr, d_blk.ptr, B, d_job.ptr, n, d_rec.ptr, d_res.ptr, d_pred.ptr, d_lev.ptr)

        def route_c():
            d_lines.upload(lines)
            c_call()
            out["c"] = np.frombuffer(d_res.to_host(np.uint8, shape=(-1,)).tobytes(), RESULT)

        # ---- route (a): tables of the four rounds, resident ------------------------------------------------------------------------------------------------
        g = IspGeom()
        assert L.vtmhip_isp_geometry(s, s, 1, g) == lib.OK
        have_a = g.partH >= 4
        if have_a:
            e, parts, pa = g.partH, g.numParts, s * g.partH          # a sub-partition: s x e or e x s, pa samples
            rl = 2 * s + 1 + 2 * e + 1                               # the lines of a sub-partition as a block of its own (the longer one first or second)
            cu_lines = lines.reshape(B, line_len)
            cu_top, cu_left = cu_lines[:, :2 * s + 1], cu_lines[:, 2 * s + 1:]
            bi = np.array([c[0] for c in cands])
            hor = np.array([c[2] == 1 for c in cands])
            orgs = np.stack([plane[(b // per_row) * s:(b // per_row) * s + s, (b % per_row) * s:(b % per_row) * s + s] for b in range(B)]).astype(np.int64)[bi]
            d_rblk, d_rjob, d_pel, d_tu = [], [], [], []
            for r in range(parts):
                rb, rj, pj, tj = (IntraBlock * n)(), (IntraJob * n)(), (PelOpJob * n)(), (TuJob * n)()
                for k, (b, m, sp) in enumerate(cands):
                    w, h = (s, e) if sp == 1 else (e, s)
                    oo = int(org_off[b]) + (r * e * STRIDE if sp == 1 else r * e)
                    rb[k] = IntraBlock(k * rl, oo, STRIDE, w, h, BD, 0)
                    rj[k] = IntraJob(k * area + r * pa, k, m)
                    pj[k] = PelOpJob(oo, k * area + r * pa, k * area + r * pa, STRIDE, w, w, w, h, BD, 0, 0, 0, 0)
                    tj[k] = TuJob(k * area + r * pa, k * area + r * pa, w, w, h, per, rem, g.typeHor if sp == 1 else g.typeVer, g.typeVer if sp == 1 else g.typeHor, BD, 0, 0, 0)
                d_rblk.append(ctx.to_device(s2n(rb))); d_rjob.append(ctx.to_device(s2n(rj))); d_pel.append(ctx.to_device(s2n(pj))); d_tu.append(ctx.to_device(s2n(tj)))    # noqa: E702
            d_rlines = ctx.alloc(2 * n * rl)
            d_apred, d_aresi, d_alev, d_arec, d_ares = (ctx.alloc(v) for v in (2 * n * area, 2 * n * area, 4 * n * area, 2 * n * area, 16 * n))

            def round_lines(r, reco):
                """the lines of sub-partition r of every candidate as a block of its own: [n, rl] (top 2w + 1, then left 2h + 1)"""
                rlines = np.zeros((n, rl), np.int16)
                for is_hor in (True, False):
                    sel = np.nonzero(hor == is_hor)[0]
                    main_cu, side_cu = (cu_top, cu_left) if is_hor else (cu_left, cu_top)
                    side = side_cu[bi[sel], r * e:r * e + 2 * e + 1]
                    if r == 0:
                        main = main_cu[bi[sel]]
                    else:
                        edge = reco[sel, r * e - 1, :] if is_hor else reco[sel, :, r * e - 1]
                        main = np.concatenate([side[:, :1], edge, np.repeat(edge[:, -1:], s, axis=1)], axis=1)
                    rlines[sel] = np.concatenate([main, side] if is_hor else [side, main], axis=1)
                return rlines

            def route_a():
                reco = np.zeros((n, s, s), np.int64)
                pred_all = np.zeros((n, s, s), np.int16)
                sums = np.zeros(n, RESULT)
                for r in range(parts):
                    d_rlines.upload(round_lines(r, reco))
                    ctx.intra_pred_batch(d_rlines.ptr, d_rblk[r].ptr, n, d_rjob[r].ptr, n, d_apred.ptr)
                    ctx.subtract_batch(d_org.ptr, d_apred.ptr, d_aresi.ptr, d_pel[r].ptr, n)
                    ctx.tu_chain_batch(d_aresi.ptr, d_tu[r].ptr, n, s, s, d_ares.ptr, d_alev.ptr, d_arec.ptr, uniform=False)
                    pred = d_apred.to_host(np.int16, shape=(n, area))[:, r * pa:(r + 1) * pa]
                    rec = d_arec.to_host(np.int16, shape=(n, area))[:, r * pa:(r + 1) * pa]
                    tr = np.frombuffer(d_ares.to_host(np.uint8, shape=(-1,)).tobytes(), TU_RESULT)
                    for is_hor in (True, False):
                        sel = np.nonzero(hor == is_hor)[0]
                        shp = (len(sel), e, s) if is_hor else (len(sel), s, e)
                        p, v = pred[sel].reshape(shp), np.clip(pred[sel].reshape(shp).astype(np.int64) + rec[sel].reshape(shp), 0, mx)
                        if is_hor:
                            reco[sel, r * e:(r + 1) * e, :], pred_all[sel, r * e:(r + 1) * e, :] = v, p
                            d = orgs[sel, r * e:(r + 1) * e, :] - v
                        else:
                            reco[sel, :, r * e:(r + 1) * e], pred_all[sel, :, r * e:(r + 1) * e] = v, p
                            d = orgs[sel, :, r * e:(r + 1) * e] - v
                        sums["sse"][sel, r] = (d * d).sum(axis=(1, 2))
                    sums["absSum"][:, r], sums["sumAbs"][:, r] = tr["absSum"], tr["sumAbs"]
                sums["numParts"] = parts
                out["a"], out["a_reco"], out["a_pred"] = sums, reco.astype(np.int16), pred_all

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
            route_c()
            if have_a:
                route_a()
        ctx.sync()
        t = {k: [] for k in ("c", "a", "c_dev")}
        for _ in range(a.reps):
            t["c"].append(wall(route_c))
            if have_a:
                t["a"].append(wall(route_a))
            t["c_dev"].append(dev(c_call))
        ctx.kernel_timing(True)
        for _ in range(a.reps):
            c_call()
        ctx.sync()
        kern_ms, launches = ctx.kernel_timing_read("isp_chain_kernel")
        ctx.kernel_timing(False)
        kernel_us = 1000.0 * kern_ms / a.reps
        lanes = lib.C.c_int()
        assert L.vtmhip_isp_chain_lanes_host(lib.C.addressof(blk_arr), B, lib.C.addressof(job_arr), n, lib.C.byref(lanes)) == lib.OK
        med = {k: float(np.median(v)) for k, v in t.items() if v}
        entry = dict(candidates=n, sub_partitions="%dx%d / %dx%d" % (g.partW, g.partH, g.partH, g.partW), lanes_per_job=lanes.value, c_us=stats(t["c"]), c_dev_us=stats(t["c_dev"]),
                     kernel_us=round(kernel_us, 1), kernel_launches=launches // a.reps, readback_pause_us=round(med["c_dev"] - kernel_us, 1),
                     readback_pause_share_of_c=round((med["c_dev"] - kernel_us) / med["c"], 3), kernel_ns_per_candidate=round(1000.0 * kernel_us / n, 1),
                     cbf_share=round(float((out["c"]["absSum"][:, :g.numParts] > 0).mean()), 3))
        if have_a:
            c_reco, c_pred = d_rec.to_host(np.int16, shape=(n, s, s)), d_pred.to_host(np.int16, shape=(n, s, s))
            same = (np.array_equal(c_reco, out["a_reco"]) and np.array_equal(c_pred, out["a_pred"]) and out["c"].tobytes() == out["a"].tobytes()
                    and np.array_equal(d_lev.to_host(np.int32, shape=(-1,)), d_alev.to_host(np.int32, shape=(-1,))))
            assert same, "the two routes disagree at %dx%d" % (s, s)
            entry.update(a_us=stats(t["a"]), a_over_c=round(med["a"] / med["c"], 2), routes_equal=True)
            for d in d_rblk + d_rjob + d_pel + d_tu + [d_rlines, d_apred, d_aresi, d_alev, d_arec, d_ares]:
                d.free()
        res["sizes"]["%dx%d" % (s, s)] = entry
        for d in (d_org, d_lines, d_blk, d_job, d_pred, d_lev, d_rec, d_res):
            d.free()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
