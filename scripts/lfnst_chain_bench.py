"""Times one full-RD level of the intra luma search with and without its LFNST candidates -- B square blocks x (3 regular modes + 1 MIP mode) predictions; blocks
8 .. 64, 10 bit, base QP 32:

  (p) vtmhip_intra_chain_batch_dev with one DCT2 candidate per prediction: what the library could do before the LFNST chain;
  (l) vtmhip_intra_chain_lfnst_batch_dev with that candidate plus lfnstIdx 1 and 2 per admissible prediction (MIP needs both sides >= 16).

    python scripts/lfnst_chain_bench.py [--blocks 256] [--reps 7]

Both sides start with the upload of the B pairs of lines and end with the download of their result records; block and job tables are resident.  Clock: the host's,
around work that ends in a stream synchronisation, after two warm-up rounds of every side; the sides alternate, `reps` times; median, min and max.  Device time: events
on the stream around the call of each side (they span the read-back of the tables and their check on the host, during which the device idles) and, from
vtmhip_kernel_timing in a pass of its own, the kernels of (l) one by one; the plain chain kernel and the LFNST chain kernel are also given per job, on the same
residuals.  Where the two sides overlap -- predictions, residuals, and levels, reconstructions and results of the plain candidates -- they are compared in full at
every size.  The matrices are the recorded ones of tests/golden/mip.npz and tests/golden/lfnst.npz.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vtm_amd import lib  # noqa: E402
from vtm_amd.device import Context, struct_array_to_numpy  # noqa: E402
from vtm_amd.lib import IntraBlock, IntraJob, IntraLfnstTuJob, IntraTuJob, MipJob  # noqa: E402

BD, QP = 10, 32
STRIDE = 4096
MODES = (0, 18, 50)
KERNELS = ("intra_resi_kernel", "mip_resi_kernel", "intra_chain_expand_kernel", "tu_chain_uni_kernel", "lfnst_expand_kernel", "lfnst_chain_kernel", "intra_chain_finish_kernel")
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
    g, z = np.load(os.path.join(ROOT, "tests", "golden", "mip.npz")), np.load(os.path.join(ROOT, "tests", "golden", "lfnst.npz"))
    ctx = Context(0)
    ctx.mip_set_tables(g["m4x4"], g["m8x8"], g["m16x16"])
    ctx.lfnst_set_tables(z["m8"], z["m4"])
    B = a.blocks
    per, rem = divmod(QP + 6 * (BD - 8), 6)
    res = dict(metric="lfnst_chain_bench", blocks=B, bitDepth=BD, qp=QP, reps=a.reps, clock="host clock around calls + stream sync (us); *_dev_us: device events", sizes={})
    for s in [int(v) for v in a.sizes.split(",")]:
        area, per_row = s * s, STRIDE // s
        plane = rng.integers(0, 1 << BD, (((B + per_row - 1) // per_row) * s, STRIDE)).astype(np.int16)
        line_len = 4 * s + 2
        lines = rng.integers(0, 1 << BD, B * line_len).astype(np.int16)
        n_intra, n_mip = B * len(MODES), B
        n_pred = n_tu = n_intra + n_mip
        lf_preds = list(range(n_pred if s >= 16 else n_intra))
        n_lf = 2 * len(lf_preds)
        blk_arr, ij, mj, tj, lj = (IntraBlock * B)(), (IntraJob * n_intra)(), (MipJob * n_mip)(), (IntraTuJob * n_tu)(), (IntraLfnstTuJob * n_lf)()
        org_off = [(b // per_row) * s * STRIDE + (b % per_row) * s for b in range(B)]
        for b in range(B):
            blk_arr[b] = IntraBlock(b * line_len, org_off[b], STRIDE, s, s, BD, 0)
            for k, mode in enumerate(MODES):
                ij[b * len(MODES) + k] = IntraJob((b * len(MODES) + k) * area, b, mode)
            mj[b] = MipJob((n_intra + b) * area, b, 0, 0)
        for p in range(n_pred):
            tj[p] = IntraTuJob(p * area, p, per, rem, lib.DCT2, lib.DCT2, 0, 0, 0)
        for k, p in enumerate(lf_preds):
            for i in (1, 2):
                lj[2 * k + i - 1] = IntraLfnstTuJob((n_tu + 2 * k + i - 1) * area, p, per, rem, i, 0)
        s2n = struct_array_to_numpy
        d_org, d_lines, d_blk, d_ij, d_mj, d_tj, d_lj = (ctx.to_device(v) for v in (plane, lines, s2n(blk_arr), s2n(ij), s2n(mj), s2n(tj), s2n(lj)))
        n_out = n_tu + n_lf
        d_pred_p, d_resi_p, d_lev_p, d_rec_p, d_res_p = (ctx.alloc(n) for n in (2 * n_pred * area, 2 * n_pred * area, 4 * n_tu * area, 2 * n_tu * area, 24 * n_tu))
        d_pred_l, d_resi_l, d_lev_l, d_rec_l, d_res_l, d_lres = (ctx.alloc(n) for n in (2 * n_pred * area, 2 * n_pred * area, 4 * n_out * area, 2 * n_out * area, 24 * n_tu,
                                                                                       24 * n_lf))
        out = {}

        def p_call():
            ctx.intra_chain_batch(d_lines.ptr, d_org.ptr, d_blk.ptr, B, d_ij.ptr, n_intra, d_mj.ptr, n_mip, d_tj.ptr, n_tu, d_pred_p.ptr, d_resi_p.ptr, d_rec_p.ptr,
                                  d_res_p.ptr, d_lev_p.ptr)

        def l_call():
            ctx.intra_chain_lfnst_batch(d_lines.ptr, d_org.ptr, d_blk.ptr, B, d_ij.ptr, n_intra, d_mj.ptr, n_mip, d_tj.ptr, n_tu, d_lj.ptr, n_lf, d_pred_l.ptr, d_resi_l.ptr,
                                        d_rec_l.ptr, d_res_l.ptr, d_lres.ptr, d_lev_l.ptr)

        def route_p():
            d_lines.upload(lines)
            p_call()
            out["p"] = np.frombuffer(d_res_p.to_host(np.uint8, shape=(-1,)).tobytes(), RESULT)

        def route_l():
            d_lines.upload(lines)
            l_call()
            out["l"] = np.frombuffer(d_res_l.to_host(np.uint8, shape=(-1,)).tobytes(), RESULT)
            out["lf"] = np.frombuffer(d_lres.to_host(np.uint8, shape=(-1,)).tobytes(), RESULT)

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
            route_p()
            route_l()
        ctx.sync()
        t = {k: [] for k in ("p", "l", "p_dev", "l_dev")}
        for _ in range(a.reps):
            t["p"].append(wall(route_p))
            t["l"].append(wall(route_l))
            t["p_dev"].append(dev(p_call))
            t["l_dev"].append(dev(l_call))
        ctx.kernel_timing(True)
        for _ in range(a.reps):
            l_call()
        split = {k: round(1000.0 * ctx.kernel_timing_read(k)[0] / a.reps, 1) for k in KERNELS}
        launches = {k: ctx.kernel_timing_read(k)[1] // a.reps for k in KERNELS}
        ctx.kernel_timing(False)
        # where the two sides overlap, in full
        same = (np.array_equal(d_pred_p.to_host(np.int16, shape=(-1,)), d_pred_l.to_host(np.int16, shape=(-1,)))
                and np.array_equal(d_resi_p.to_host(np.int16, shape=(-1,)), d_resi_l.to_host(np.int16, shape=(-1,)))
                and np.array_equal(d_lev_p.to_host(np.int32, shape=(-1,)), d_lev_l.to_host(np.int32, shape=(-1,))[:n_tu * area])
                and np.array_equal(d_rec_p.to_host(np.int16, shape=(-1,)), d_rec_l.to_host(np.int16, shape=(-1,))[:n_tu * area]) and np.array_equal(out["p"], out["l"]))
        assert same, "the two sides disagree at %dx%d" % (s, s)
        med = {k: float(np.median(v)) for k, v in t.items()}
        res["sizes"]["%dx%d" % (s, s)] = dict(predictions=n_pred, plain_jobs=n_tu, lfnst_jobs=n_lf, p_us=stats(t["p"]), l_us=stats(t["l"]), l_over_p=round(med["l"] / med["p"], 2),
                                              p_dev_us=stats(t["p_dev"]), l_dev_us=stats(t["l_dev"]), l_minus_p_dev_us=round(med["l_dev"] - med["p_dev"], 1),
                                              l_kernels_us=split, l_kernel_launches=launches, l_kernels_sum_us=round(sum(split.values()), 1),
                                              plain_chain_ns_per_job=round(1000.0 * split["tu_chain_uni_kernel"] / n_tu, 1),
                                              lfnst_chain_ns_per_job=round(1000.0 * split["lfnst_chain_kernel"] / n_lf, 1),
                                              lfnst_cbf_share=round(float((out["lf"]["absSum"] > 0).mean()), 3), plain_cbf_share=round(float((out["l"]["absSum"] > 0).mean()), 3),
                                              overlap_equal=True)
        for d in (d_org, d_lines, d_blk, d_ij, d_mj, d_tj, d_lj, d_pred_p, d_resi_p, d_lev_p, d_rec_p, d_res_p, d_pred_l, d_resi_l, d_lev_l, d_rec_l, d_res_l, d_lres):
            d.free()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
