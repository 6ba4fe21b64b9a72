"""Raster pruning on content the bound does not favour: the uniform 128x128 uni batch (vtmhip_xMotionEstimation_batch_dev, zero predictors, search range 96) of a
3840x2160 picture of the hard clip (synth.gen_frames_hard, two textures moving in opposite directions + sigma-10 noise) at dPOC 2 and 4, and of the benchmark's clip
(synth.gen_frames, a pure pan; dPOC 4 -- at dPOC 2 the diamond reaches the motion and no search comes to a scan) for contrast -- with the box sums attached and without.  Prints, per clip: ms of the batch and of its tz_raster_cols_kernel launch (HIP
events), ms of the two tz_search launches together (first and resume; VTMHIP_TZ_ROUND_BOUND=0 in the environment: without the round bound), the round
statistic (vtmhip_tz_round_stats of one batch), ms of the box-sum pass, the statistic (share of scans skipped / reduced, grid points evaluated / total) and a checksum of the records (equal on and off)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import me_util
    from vtm_amd.device import Context
    from vtm_amd.lib import MeCfg, MeJob, MeOut, PicParams
    W, H = (int(v) for v in os.environ.get("PRUNE_BENCH_SIZE", "3840x2160").split("x"))
    w = h = 128
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    cfg = MeCfg(4, 1, 1, 0, 1, 0, 1, 1, 0, 0)      # the benchmark's uni configuration: FastInterSearchMode 1, no extended settings, uniform all-uni rows
    pic = PicParams(W, H, 128, 10, 8)
    out = {}
    for name, hard, t_cur in (("hard_dpoc2", True, 2), ("hard_dpoc4", True, 4), ("bench_clip_dpoc4", False, 4)):
        scene = me_util.Scene(W, H, hard=hard, t_ref=0, t_cur=t_cur)
        xs, ys = np.meshgrid(np.arange(0, W - w + 1, w), np.arange(0, H - h + 1, h))
        xs, ys = xs.reshape(-1), ys.reshape(-1)
        n = xs.size
        j = np.zeros(n, np.dtype(MeJob))
        j["orgOff"], j["orgStride"] = ys * W + xs, W
        j["refOff"], j["refStride"] = scene.ref_off + ys * scene.ref_stride + xs, scene.ref_stride
        j["puX"], j["puY"], j["width"], j["height"] = xs, ys, w, h
        j["numAmvpCand"], j["mvpIdxBits"], j["bits"], j["searchRange"], j["motionLambda"] = 2, 1, 6, 96, 31.3
        j["amvpCand"][:, 1, 0] = 16
        d_cur, d_ref, d_oth = ctx.to_device(scene.cur), ctx.to_device(scene.ref_buf), ctx.to_device(np.zeros(1, np.int16))
        d_jobs, d_res, d_sums = ctx.to_device(j.view(np.uint8)), ctx.alloc(C.sizeof(MeOut) * n), ctx.alloc(2 * scene.ref_buf.size)
        row = dict(scans=int(n))
        for mode in ("off", "on"):
            def once():
                if mode == "on":
                    ctx.tz_box_sums(d_ref.ptr, d_sums.ptr, scene.ref_off, scene.ref_stride, W, H, scene.margin)
                    ctx.tz_attach_sums(d_ref.ptr, d_sums.ptr, W, H, scene.margin)
                ctx.motion_estimation_batch(pic, cfg, d_cur.ptr, d_ref.ptr, d_oth.ptr, d_jobs.ptr, n, w, h, d_res.ptr)
                ctx.tz_attach_sums(None, None)
            once()
            torch.cuda.synchronize()
            reps = 5
            ctx.tz_prune_stats(reset=True)
            ctx.tz_round_stats(reset=True)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(reps):
                once()
            ev[1].record()
            torch.cuda.synchronize()
            st = ctx.tz_prune_stats()
            rs = {k: v // reps for k, v in ctx.tz_round_stats().items()}
            ctx.kernel_timing(True)
            once()
            raster_ms, _ = ctx.kernel_timing_read("tz_raster_cols_kernel")
            box_ms, _ = ctx.kernel_timing_read("box_sum8_kernel")
            search_ms, search_n = ctx.kernel_timing_read("tz_search_kernel")
            ctx.kernel_timing(False)
            res = np.frombuffer(d_res.to_host(np.uint8).tobytes(), np.dtype(MeOut))
            row[mode] = dict(batch_ms=round(ev[0].elapsed_time(ev[1]) / reps, 3), raster_ms=round(raster_ms, 3), search_ms=round(search_ms, 3), search_launches=search_n, round_stats=rs, box_sum_ms=round(box_ms, 3),
                             listed=st["listed"] // reps, skipped_share=round(st["skipped"] / max(1, st["listed"]), 3), reduced_share=round(st["reduced"] / max(1, st["listed"]), 3),
                             accepted_share=round(st["accepted"] / max(1, st["listed"]), 3), points_evaluated=st["points_evaluated"] // reps, points_total=st["points_total"] // reps,
                             checksum=int(res["cost"].astype(np.uint64).sum() % (1 << 31)))
        assert row["on"]["checksum"] == row["off"]["checksum"], row
        out[name] = row
        print(name, row, flush=True)
        for d in (d_cur, d_ref, d_oth, d_jobs, d_res, d_sums):
            d.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
