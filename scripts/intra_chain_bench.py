"""Times one full-RD level of the intra luma search -- B square blocks x (3 regular modes + 1 MIP mode) predictions x the transform candidates DCT2-DCT2 and, up
to 32x32, DST7-DST7; blocks 8 .. 64, 10 bit -- on the two routes the library offers:

  (a) the route before vtmhip_intra_chain_batch_dev, for the same jobs: vtmhip_intra_pred_batch_dev + vtmhip_mip_pred_batch_dev, vtmhip_subtract_batch_dev,
      vtmhip_tu_chain_batch_dev (uniformSize = 1: the caller knows its level has one shape), the download of the predictions and of the reconstructed residual,
      then reconstruction, clip and SSE in numpy (the original blocks are gathered once, outside the clock);
  (c) the one new call and the download of its result records.

    python scripts/intra_chain_bench.py [--blocks 256] [--reps 7]

Both routes start with the upload of the B pairs of lines; block and job tables are resident.  Clock: the host's, around work that ends in a stream synchronisation,
after two warm-up rounds of every side; the sides alternate, `reps` times; median, min and max.  Device time: events on the stream around each of the three device
steps of (a) and around the call of (c) -- the latter spans the read-back of the tables and their check on the host, during which the device idles -- and, from
vtmhip_kernel_timing in a pass of its own, the kernels of (c) one by one.  Predictions, residuals, levels, reconstructions and SSEs of the two routes are compared
in full at every size.  The matrices are the recorded ones of tests/golden/mip.npz.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vtm_amd import lib  # noqa: E402
from vtm_amd.device import Context, intra_chain_make_tu_jobs, struct_array_to_numpy  # noqa: E402
from vtm_amd.lib import IntraBlock, IntraJob, IntraTuJob, MipJob, PelOpJob  # noqa: E402

BD, QP = 10, 32
STRIDE = 4096
MODES = (0, 18, 50)
KERNELS = ("intra_resi_kernel", "mip_resi_kernel", "intra_chain_expand_kernel", "tu_chain_uni_kernel", "intra_chain_finish_kernel")
RESULT = np.dtype([("sse", "<u8"), ("sseResi", "<u8"), ("sumAbs", "<i4"), ("absSum", "<i4")])


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
    per, rem = divmod(QP + 6 * (BD - 8), 6)
    res = dict(metric="intra_chain_bench", blocks=B, bitDepth=BD, qp=QP, reps=a.reps, clock="host clock around calls + stream sync (us); *_dev_us: device events", sizes={})
    for s in [int(v) for v in a.sizes.split(",")]:
        area, per_row = s * s, STRIDE // s
        cands = [(lib.DCT2, lib.DCT2)] + ([(lib.DST7, lib.DST7)] if s <= 32 else [])
        plane = rng.integers(0, 1 << BD, (((B + per_row - 1) // per_row) * s, STRIDE)).astype(np.int16)
        line_len = 4 * s + 2
        lines = rng.integers(0, 1 << BD, B * line_len).astype(np.int16)
        n_intra, n_mip = B * len(MODES), B
        n_pred, n_tu = n_intra + n_mip, (n_intra + n_mip) * len(cands)
        blk_arr, ij, mj, tj, sj = (IntraBlock * B)(), (IntraJob * n_intra)(), (MipJob * n_mip)(), (IntraTuJob * n_tu)(), (PelOpJob * n_pred)()
        org_off = [(b // per_row) * s * STRIDE + (b % per_row) * s for b in range(B)]
        for b in range(B):
            blk_arr[b] = IntraBlock(b * line_len, org_off[b], STRIDE, s, s, BD, 0)
            for k, mode in enumerate(MODES):
                ij[b * len(MODES) + k] = IntraJob((b * len(MODES) + k) * area, b, mode)
            mj[b] = MipJob((n_intra + b) * area, b, 0, 0)
        pred_block = np.array([j.block for j in ij] + [j.block for j in mj])
        for p in range(n_pred):
            sj[p] = PelOpJob(org_off[pred_block[p]], p * area, p * area, STRIDE, s, s, s, s, BD, 0, 0, 0, 0)
            for k, (th, tv) in enumerate(cands):
                tj[p * len(cands) + k] = IntraTuJob((p * len(cands) + k) * area, p, per, rem, th, tv, 0, 0, 0)
        tu_pred = np.array([t.pred for t in tj])
        xj, mw, mh, uni = intra_chain_make_tu_jobs(blk_arr, ij, mj, tj)
        assert (mw, mh, uni) == (s, s, 1)
        org = np.stack([plane[o // STRIDE:o // STRIDE + s, o % STRIDE:o % STRIDE + s].reshape(-1) for o in org_off]).astype(np.int64)
        s2n = struct_array_to_numpy
        d_org, d_lines, d_blk, d_ij, d_mj, d_tj, d_sj, d_xj = (ctx.to_device(v) for v in (plane, lines, s2n(blk_arr), s2n(ij), s2n(mj), s2n(tj), s2n(sj), s2n(xj)))
        d_pred_a, d_resi_a, d_lev_a, d_rec_a, d_res_a = (ctx.alloc(n) for n in (2 * n_pred * area, 2 * n_pred * area, 4 * n_tu * area, 2 * n_tu * area, 16 * n_tu))
        d_pred_c, d_resi_c, d_lev_c, d_rec_c, d_res_c = (ctx.alloc(n) for n in (2 * n_pred * area, 2 * n_pred * area, 4 * n_tu * area, 2 * n_tu * area, 24 * n_tu))
        out = {}

        def a_pred():
            ctx.intra_pred_batch(d_lines.ptr, d_blk.ptr, B, d_ij.ptr, n_intra, d_pred_a.ptr)
            ctx.mip_pred_batch(d_lines.ptr, d_blk.ptr, B, d_mj.ptr, n_mip, d_pred_a.ptr)

        def a_sub():
            ctx.subtract_batch(d_org.ptr, d_pred_a.ptr, d_resi_a.ptr, d_sj.ptr, n_pred)

        def a_chain():
            ctx.tu_chain_batch(d_resi_a.ptr, d_xj.ptr, n_tu, s, s, d_res_a.ptr, d_lev_a.ptr, d_rec_a.ptr, uniform=True)

        def route_a():
            d_lines.upload(lines)
            a_pred()
            a_sub()
            a_chain()
            pred = d_pred_a.to_host(np.int16, shape=(n_pred, area))
            rec = d_rec_a.to_host(np.int16, shape=(n_tu, area))
            reco = np.clip(pred[tu_pred].astype(np.int32) + rec, 0, (1 << BD) - 1)
            d = org[pred_block[tu_pred]] - reco
            out["a"] = (reco.astype(np.int16), (d * d).sum(1).astype(np.uint64))

        def c_call():
            ctx.intra_chain_batch(d_lines.ptr, d_org.ptr, d_blk.ptr, B, d_ij.ptr, n_intra, d_mj.ptr, n_mip, d_tj.ptr, n_tu, d_pred_c.ptr, d_resi_c.ptr, d_rec_c.ptr,
                                  d_res_c.ptr, d_lev_c.ptr)

        def route_c():
            d_lines.upload(lines)
            c_call()
            out["c"] = np.frombuffer(d_res_c.to_host(np.uint8, shape=(-1,)).tobytes(), RESULT)

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
        t = {k: [] for k in ("a", "c", "a_pred_dev", "a_sub_dev", "a_chain_dev", "c_dev")}
        for _ in range(a.reps):
            t["a"].append(wall(route_a))
            t["c"].append(wall(route_c))
            for k, fn in (("a_pred_dev", a_pred), ("a_sub_dev", a_sub), ("a_chain_dev", a_chain), ("c_dev", c_call)):
                t[k].append(dev(fn))
        ctx.kernel_timing(True)
        for _ in range(a.reps):
            c_call()
        split = {k: round(1000.0 * ctx.kernel_timing_read(k)[0] / a.reps, 1) for k in KERNELS}
        ctx.kernel_timing(False)
        # the two routes in full
        reco_a, sse_a = out["a"]
        same = (np.array_equal(d_pred_a.to_host(np.int16, shape=(-1,)), d_pred_c.to_host(np.int16, shape=(-1,)))
                and np.array_equal(d_resi_a.to_host(np.int16, shape=(-1,)), d_resi_c.to_host(np.int16, shape=(-1,)))
                and np.array_equal(d_lev_a.to_host(np.int32, shape=(-1,)), d_lev_c.to_host(np.int32, shape=(-1,)))
                and np.array_equal(reco_a.reshape(-1), d_rec_c.to_host(np.int16, shape=(-1,))) and np.array_equal(sse_a, out["c"]["sse"]))
        ra = np.frombuffer(d_res_a.to_host(np.uint8, shape=(-1,)).tobytes(), np.dtype([("sse", "<u8"), ("sumAbs", "<i4"), ("absSum", "<i4")]))
        same = same and all(np.array_equal(ra[k], out["c"][q]) for k, q in (("sse", "sseResi"), ("sumAbs", "sumAbs"), ("absSum", "absSum")))
        assert same, "the two routes disagree at %dx%d" % (s, s)
        med = {k: float(np.median(v)) for k, v in t.items()}
        a_dev_sum = med["a_pred_dev"] + med["a_sub_dev"] + med["a_chain_dev"]
        res["sizes"]["%dx%d" % (s, s)] = dict(predictions=n_pred, tu_jobs=n_tu, cands_per_prediction=len(cands), download_bytes_a=2 * (n_pred + n_tu) * area,
                                              download_bytes_c=24 * n_tu, a_us=stats(t["a"]), c_us=stats(t["c"]), a_over_c=round(med["a"] / med["c"], 2),
                                              a_pred_dev_us=stats(t["a_pred_dev"]), a_sub_dev_us=stats(t["a_sub_dev"]), a_chain_dev_us=stats(t["a_chain_dev"]),
                                              a_dev_sum_us=round(a_dev_sum, 1), c_dev_us=stats(t["c_dev"]), c_kernels_us=split, c_kernels_sum_us=round(sum(split.values()), 1),
                                              clipped_samples=int((reco_a == 0).sum() + (reco_a == (1 << BD) - 1).sum()), results_equal=True)
        for d in (d_org, d_lines, d_blk, d_ij, d_mj, d_tj, d_sj, d_xj, d_pred_a, d_resi_a, d_lev_a, d_rec_a, d_res_a, d_pred_c, d_resi_c, d_lev_c, d_rec_c, d_res_c):
            d.free()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
