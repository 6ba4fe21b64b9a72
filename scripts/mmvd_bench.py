"""Times the MMVD candidates of one merge level -- B CUs of one shape, two base candidates each (a bi base on equal and opposite POC distances, so its first three
steps are BDOF candidates where the shape allows it, and a list-0 base), all 64 indices tested, 10 bit, SATD:

  (f) vtmhip_mmvd_cand_satd_batch_dev: the candidates derived on the device, the plain ones predicted and reduced to their cost in one kernel, the BDOF ones expanded;
  (c) the composition a hook could build before that entry: the candidates derived on the host (tests/mmvd_util.py, outside the timed window -- an encoder would do it
      in C++) and 64 vtmhip_pred_job rows per CU, split by the kind of prediction, through vtmhip_merge_cand_satd_batch_dev with its uniform distortion stage: the
      predictions go to global memory and are read back for the distortion.

    python scripts/mmvd_bench.py [--blocks 256] [--reps 9] [--inner 10]

Planes and job tables are resident; a measurement is `inner` calls of one route and a stream synchronisation under the host's clock, divided by `inner`, after two
warm-up rounds of both routes; the routes alternate, `reps` times; median, min and max per call in microseconds.  spread = ( max - min ) / median of a route's own
repetitions.  (f) synchronises the stream once per call by itself (it reads its job table back); (c) does not.  The costs of the two routes are compared in full.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mmvd_util as mu  # noqa: E402
from vtm_amd.device import Context, struct_array_to_numpy as s2n  # noqa: E402
from vtm_amd.lib import MmvdCand, MmvdJob, PicParams, PredJob  # noqa: E402

BD, CTU, MARGIN, SLACK = 10, 128, 160, 2048
PIC_W, PIC_H = 2048, 1024
REF_STRIDE = PIC_W + 2 * MARGIN
PLANE = (PIC_H + 2 * MARGIN) * REF_STRIDE


def stats(v):
    return dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1), spread=round((max(v) - min(v)) / float(np.median(v)), 3))


def ref_off(l, x, y):
    return SLACK + l * PLANE + (MARGIN + y) * REF_STRIDE + MARGIN + x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", type=str, default="8x8,16x8,16x16,32x32,64x64,128x128")
    a = ap.parse_args()
    rng = np.random.default_rng(11)
    ctx = Context(0)
    pic = PicParams(PIC_W, PIC_H, CTU, BD)
    org = rng.integers(0, 1 << BD, (PIC_H, PIC_W)).astype(np.int16)
    refs = np.concatenate([np.zeros(SLACK, np.int16), rng.integers(0, 1 << BD, 2 * PLANE).astype(np.int16), np.zeros(SLACK, np.int16)])
    d_org, d_ref = ctx.to_device(org), ctx.to_device(refs)
    res = dict(metric="mmvd_bench", route_env=os.environ.get("VTMHIP_MMVD_FUSED", "unset"), blocks=a.blocks, bitDepth=BD, reps=a.reps, inner=a.inner, clock="host clock around `inner` calls + stream sync, per call (us)", sizes={})
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        per_row = PIC_W // w
        B = min(a.blocks, per_row * (PIC_H // h))
        jobs = []
        for b in range(B):
            x, y = (b % per_row) * w, (b // per_row) * h
            mv = rng.integers(-64, 65, 6)
            bases = [mu.make_base(mv=((int(mv[0]), int(mv[1])), (int(mv[2]), int(mv[3]))), ref_idx=(0, 0), poc_diff=(-2, 2)),
                     mu.make_base(mv=((int(mv[4]), int(mv[5])), (0, 0)), ref_idx=(1, -1), poc_diff=(-4, 0))]
            for s in bases:
                s["ref_off"], s["ref_stride"] = [ref_off(0, x, y), ref_off(1, x, y)], [REF_STRIDE, REF_STRIDE]
            jobs.append(mu.make_job(w, h, bases, pos=(x, y), bd=BD, org_off=y * PIC_W + x, org_stride=PIC_W))
        job_arr = (MmvdJob * B)(*[mu.to_struct(j) for j in jobs])
        # route (c): the host's candidates as prediction jobs, plain and BDOF, and where each lands in the fused call's table
        plain, bdof, slot_p, slot_b = [], [], [], []
        for i, j in enumerate(jobs):
            for c, d in enumerate(mu.derive_all(j, (PIC_W, PIC_H, CTU))):
                assert d["kind"] != mu.NOT_TESTED and d["bcw"] == mu.BCW_DEFAULT
                s = j["bases"][c // 32]
                k = len(plain) + len(bdof)
                p = PredJob(j["org_off"], (C.c_int64 * 2)(*s["ref_off"]), k * w * h, 0, PIC_W, (C.c_int32 * 2)(*s["ref_stride"]), w, 0,
                            ((C.c_int32 * 2) * 2)((C.c_int32 * 2)(*d["pred_mv"][0]), (C.c_int32 * 2)(*d["pred_mv"][1])), w, h, d["pred_mode"], 0, BD, d["alt_hpel"], 0, 0, 0)
                (bdof if d["kind"] == mu.BDOF else plain).append(p)
                (slot_b if d["kind"] == mu.BDOF else slot_p).append(64 * i + c)
        n_p, n_b = len(plain), len(bdof)
        d_jobs = ctx.to_device(s2n(job_arr))
        d_plain = ctx.to_device(s2n((PredJob * n_p)(*plain)))
        d_bdof = ctx.to_device(s2n((PredJob * max(n_b, 1))(*bdof)))
        d_cand, d_dist_f = ctx.alloc(B * 64 * C.sizeof(MmvdCand)), ctx.alloc(B * 64 * 8)
        d_pred, d_dist_c = ctx.alloc(2 * (n_p + n_b) * w * h), ctx.alloc(8 * (n_p + n_b))

        def route_f():
            ctx.mmvd_cand_satd_batch(pic, d_org.ptr, d_ref.ptr, d_jobs.ptr, B, w, h, d_cand.ptr, d_dist_f.ptr)

        def route_c():
            ctx.merge_cand_satd_batch(pic, d_org.ptr, d_ref.ptr, d_pred.ptr, d_plain.ptr, n_p, d_bdof.ptr if n_b else 0, n_b, 0, 0, 0, w, h, d_dist_c.ptr, uniform=True)

        def wall(fn):
            ctx.sync()
            t = time.perf_counter()
            for _ in range(a.inner):
                fn()
            ctx.sync()
            return (time.perf_counter() - t) * 1e6 / a.inner

        for _ in range(2):
            route_f()
            route_c()
        ctx.sync()
        got_f, got_c = d_dist_f.to_host(np.uint64), d_dist_c.to_host(np.uint64)
        assert np.array_equal(got_f[np.array(slot_p + slot_b, np.int64)], got_c), "the two routes disagree at %s" % size
        def dev(fn):
            ctx.timer_start()
            fn()
            return ctx.timer_stop_ms() * 1000.0

        t = dict(f=[], c=[], f_dev=[], c_dev=[])
        for _ in range(a.reps):
            t["f"].append(wall(route_f))
            t["c"].append(wall(route_c))
            t["f_dev"].append(dev(route_f))
            t["c_dev"].append(dev(route_c))
        ctx.kernel_timing(True)
        for _ in range(a.reps):
            route_f()
        ctx.sync()
        kern_ms, launches = ctx.kernel_timing_read("mmvd_fused_kernel")
        ctx.kernel_timing(False)
        f, c = stats(t["f"]), stats(t["c"])
        res["sizes"][size] = dict(cus=B, candidates=64 * B, bdof_candidates=n_b, lanes_per_block=ctx.L.vtmhip_mc_lanes_per_block(w, h), new_call_us=f, composition_us=c,
                                  new_call_dev_us=stats(t["f_dev"]), composition_dev_us=stats(t["c_dev"]), fused_kernel_us=round(1000.0 * kern_ms / a.reps, 1),
                                  fused_kernel_launches=launches // a.reps, composition_over_new_call=round(c["median"] / f["median"], 2),
                                  new_call_ns_per_candidate=round(1000.0 * f["median"] / (64 * B), 1),
                                  new_call_not_slower_within_spread=bool(f["median"] <= c["median"] * (1.0 + max(f["spread"], c["spread"]))), routes_equal=True)
        for d in (d_jobs, d_plain, d_bdof, d_cand, d_dist_f, d_pred, d_dist_c):
            d.free()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
