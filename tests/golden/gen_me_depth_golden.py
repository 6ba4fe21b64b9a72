"""Generates tests/golden/me_depth.npz: results of the REAL reference members (oracle/_ref/libvtmref.so) InterSearch::xTZSearch and InterSearch::xMotionEstimation
at 8 and 12 bits on a natural and a saturated scene, under the motion lambdas the reference derives from QP 22 .. 63 at the depth (xTZSearch: also 6e5 / 2e7 / 3e9).

    python tests/golden/gen_me_depth_golden.py

The pictures are not stored: they are me_util.DeepScene( 416, 240, hard=True, bit_depth ) and me_util.SaturatedScene( 416, 240, bit_depth, seed ), whose sums are
recorded in `plane_sums` so that a replay notices when a generator changes.  Jobs are the JSON of the me_util job dictionaries; results are int64 rows:
tz (mvX, mvY, cost, dist), mest (mvHor, mvVer, mvPredHor, mvPredVer, mvpIdx, bits, cost, intX, intY) with intX / intY of bi rows stored as 0."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import me_util  # noqa: E402
import oracle_lib as ol  # noqa: E402

CFGV = (4, 1, 1, 0, 1)
SCENES = [(bd, sat) for bd in (8, 12) for sat in (0, 1)]


def scene_of(bd, sat):
    return me_util.SaturatedScene(416, 240, bd, seed=60 + bd) if sat else me_util.DeepScene(416, 240, hard=True, bit_depth=bd)


def plane_sum(scene):
    return [int(scene.cur.astype(np.int64).sum()), int(scene.ref_buf.astype(np.int64).sum())]


def tz_jobs(scene, bd, sat):
    lams = me_util.real_lambdas(bd)
    if sat:
        return me_util.random_tz_jobs(scene, 40, seed=4100 + bd, lams=lams + me_util.EDGE) + me_util.random_tz_jobs(scene, 35, seed=4200 + bd, sizes=me_util.BIG, lams=lams)
    return me_util.random_tz_jobs(scene, 75, seed=4000 + bd, lams=lams + me_util.EDGE)


def mest_jobs(scene, bd, sat):
    jobs = me_util.random_mest_jobs(scene, 80, seed=4300 + bd + sat, lams=me_util.real_lambdas(bd), bcws=(0, -2, 3, 5, 10))
    return [j for j in jobs if not (sat and me_util.simd_had4_split(j, CFGV, bd))]


def main():
    R = ol.ref()
    cfg = ol.MestCfg(*CFGV)
    out = {"scenes": np.array(SCENES, np.int32), "cfg": np.array(CFGV, np.int32)}
    sums = []
    for bd, sat in SCENES:
        scene = scene_of(bd, sat)
        sums.append(plane_sum(scene))
        jobs, rows = tz_jobs(scene, bd, sat), []
        for j in jobs:
            org = np.ascontiguousarray(scene.cur[j["y"]:j["y"] + j["h"], j["x"]:j["x"] + j["w"]])
            c, t, r = me_util.oracle_ctx(scene, j, org), me_util.oracle_tz_job(j), ol.MeResult()
            R.ref_tz_search(C.byref(c), C.byref(t), C.byref(r))
            rows.append((r.mvX, r.mvY, r.cost, r.dist))
        out["tz_jobs_%d_%d" % (bd, sat)] = np.array([json.dumps(j) for j in jobs])
        out["tz_res_%d_%d" % (bd, sat)] = np.array(rows, np.int64)
        jobs, rows = mest_jobs(scene, bd, sat), []
        for j in jobs:
            keep = []
            t, r = me_util.oracle_mest_job(scene, j, keep), ol.MestResult()
            R.ref_motion_estimation(C.byref(cfg), C.byref(t), C.byref(r))
            rows.append(r.key() + ((0, 0) if j["bi"] else (r.intX, r.intY)))
        out["mest_jobs_%d_%d" % (bd, sat)] = np.array([json.dumps(j) for j in jobs])
        out["mest_res_%d_%d" % (bd, sat)] = np.array(rows, np.int64)
        print(bd, sat, len(out["tz_jobs_%d_%d" % (bd, sat)]), "tz,", len(jobs), "mest")
    out["plane_sums"] = np.array(sums, np.int64)
    np.savez_compressed(os.path.join(HERE, "me_depth.npz"), **out)


if __name__ == "__main__":
    main()
