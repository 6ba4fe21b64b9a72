"""Times the CIIP candidates of one merge level -- B CUs of one shape, four candidates each, 10 bit, SATD, LMCS off (the composition has no inverse-LUT step):

  (f) vtmhip_ciip_cand_satd_batch_dev: planar once per CU and, per candidate, prediction, blend and SATD in one kernel; nothing but the costs is stored;
  (c) the composition a hook could build from the other entries: vtmhip_motion_compensation_batch_dev into a plane, vtmhip_ciip_blend_batch_dev with luma jobs over
      it, vtmhip_dist_batch_dev: the predictions go to global memory, are blended there and read back for the distortion.

Both routes run twice: with four bi candidates per CU (mode 2: the motion compensation is part of the work) and with the four inter blocks given (mode 3: (f) copies
them into LDS; (c) blends in place, so it first copies the blocks, which the RD stage still needs, into its plane: motion-compensation jobs with a zero vector
over the given blocks, the copy an encoder hook has at hand).

    python scripts/ciip_bench.py [--blocks 256] [--reps 9] [--inner 10]

Planes, lines and job tables are resident; a measurement is `inner` calls of one route and a stream synchronisation under the host's clock, divided by `inner`, after
two warm-up rounds of both routes; the routes alternate, `reps` times; median, min and max per call in microseconds.  spread = ( max - min ) / median of a route's
own repetitions.  Neither route synchronises by itself.  The costs of the two routes are compared in full before timing.  Prints one JSON line."""
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

import ciip_util as cu  # noqa: E402
from vtm_amd import lib  # noqa: E402
from vtm_amd.device import Context, struct_array_to_numpy as s2n  # noqa: E402
from vtm_amd.lib import CiipBlendJob, CiipJob, DistJob, PredJob  # noqa: E402

BD, MARGIN, SLACK = 10, 160, 2048
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
    ap.add_argument("--sizes", type=str, default="8x8,16x16,32x32,64x64")
    a = ap.parse_args()
    rng = np.random.default_rng(12)
    ctx = Context(0)
    org = rng.integers(0, 1 << BD, (PIC_H, PIC_W)).astype(np.int16)
    refs = np.concatenate([np.zeros(SLACK, np.int16), rng.integers(0, 1 << BD, 2 * PLANE).astype(np.int16), np.zeros(SLACK, np.int16)])
    d_org, d_ref = ctx.to_device(org), ctx.to_device(refs)
    res = dict(metric="ciip_bench", blocks=a.blocks, bitDepth=BD, candidates_per_cu=4, reps=a.reps, inner=a.inner,
               clock="host clock around `inner` calls + stream sync, per call (us)", sizes={})
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        per_row = PIC_W // w
        B = min(a.blocks, per_row * (PIC_H // h))
        n_line, area = 2 * w + 2 * h + 2, w * h
        lines = rng.integers(0, 1 << BD, B * n_line).astype(np.int16)
        given = rng.integers(0, 1 << BD, 4 * B * area).astype(np.int16)
        jobs = {2: [], 3: []}
        pred_jobs, copy_jobs, blend_jobs, dist_jobs = [], [], [], []
        for b in range(B):
            x, y = (b % per_row) * w, (b // per_row) * h
            for mode in (2, 3):
                cands = []
                for k in range(4):
                    mv = rng.integers(-64, 65, 4) if mode == 2 else np.zeros(4, np.int64)
                    cands.append(cu.make_cand(mode=mode, ref_off=(ref_off(0, x, y), ref_off(1, x, y)), ref_stride=(REF_STRIDE, REF_STRIDE),
                                              mv=((int(mv[0]), int(mv[1])), (int(mv[2]), int(mv[3]))), src_off=(4 * b + k) * area, src_stride=w))
                jobs[mode].append(cu.make_job(w, h, BD, cands, left=b & 1, above=(b >> 1) & 1, line_off=b * n_line, org_off=y * PIC_W + x, org_stride=PIC_W))
            for k, c in enumerate(jobs[2][-1]["cands"]):
                at = (4 * b + k) * area
                pred_jobs.append(PredJob(0, (C.c_int64 * 2)(*c["ref_off"]), at, 0, PIC_W, (C.c_int32 * 2)(*c["ref_stride"]), w, 0,
                                         ((C.c_int32 * 2) * 2)((C.c_int32 * 2)(*c["mv"][0]), (C.c_int32 * 2)(*c["mv"][1])), w, h, 2, 0, BD, 0, 0, 0, 0))
                copy_jobs.append(PredJob(0, (C.c_int64 * 2)(at, at), at, 0, PIC_W, (C.c_int32 * 2)(w, w), w, 0, ((C.c_int32 * 2) * 2)(), w, h, 0, 0, BD, 0, 0, 0, 0))
                blend_jobs.append(cu.blend_struct(w, h, BD, b * n_line, at, w, left=b & 1, above=(b >> 1) & 1))
                dist_jobs.append(DistJob(y * PIC_W + x, at, PIC_W, w, w, h, 0, lib.DIST_SATD))
        n = 4 * B
        d_line, d_given = ctx.to_device(lines), ctx.to_device(given)
        d_jobs = {m: ctx.to_device(s2n((CiipJob * B)(*[cu.to_struct(j) for j in jobs[m]]))) for m in (2, 3)}
        d_cj = ctx.to_device(s2n((PredJob * n)(*copy_jobs)))
        d_pj, d_bj, d_dj = ctx.to_device(s2n((PredJob * n)(*pred_jobs))), ctx.to_device(s2n((CiipBlendJob * n)(*blend_jobs))), ctx.to_device(s2n((DistJob * n)(*dist_jobs)))
        d_plane, d_dist_f, d_dist_c = ctx.alloc(2 * n * area), ctx.alloc(8 * n), ctx.alloc(8 * n)

        def route_f(mode):
            ctx.ciip_cand_satd_batch(d_ref.ptr, d_line.ptr, d_org.ptr, d_given.ptr, d_jobs[mode].ptr, B, w, h, d_dist_f.ptr)

        def route_c(mode):
            if mode == 2:
                ctx.motion_compensation_batch(0, d_ref.ptr, d_plane.ptr, 0, d_pj.ptr, n, w, h)
            else:
                ctx.motion_compensation_batch(0, d_given.ptr, d_plane.ptr, 0, d_cj.ptr, n, w, h)
            ctx.ciip_blend_batch(d_line.ptr, d_plane.ptr, d_bj.ptr, n)
            ctx.dist_batch(d_org.ptr, d_plane.ptr, d_dj.ptr, n, d_dist_c.ptr)

        def wall(fn, mode):
            ctx.sync()
            t = time.perf_counter()
            for _ in range(a.inner):
                fn(mode)
            ctx.sync()
            return (time.perf_counter() - t) * 1e6 / a.inner

        entry = dict(cus=B, candidates=n, lanes_per_block=ctx.L.vtmhip_mc_lanes_per_block(w, h))
        for mode, name in ((2, "bi"), (3, "given")):
            for _ in range(2):
                route_f(mode)
                route_c(mode)
            ctx.sync()
            got_f, got_c = d_dist_f.to_host(np.uint64), d_dist_c.to_host(np.uint64)
            assert np.array_equal(got_f, got_c) and got_f.max() < cu.NO_COST, "the two routes disagree at %s, mode %d" % (size, mode)
            t = dict(f=[], c=[])
            for _ in range(a.reps):
                t["f"].append(wall(route_f, mode))
                t["c"].append(wall(route_c, mode))
            f, c = stats(t["f"]), stats(t["c"])
            entry[name] = dict(new_call_us=f, composition_us=c, composition_over_new_call=round(c["median"] / f["median"], 2),
                               new_call_ns_per_candidate=round(1000.0 * f["median"] / n, 1),
                               new_call_not_slower_within_spread=bool(f["median"] <= c["median"] * (1.0 + max(f["spread"], c["spread"]))), routes_equal=True)
        res["sizes"][size] = entry
        for d in (d_line, d_given, d_jobs[2], d_jobs[3], d_pj, d_cj, d_bj, d_dj, d_plane, d_dist_f, d_dist_c):
            d.free()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
