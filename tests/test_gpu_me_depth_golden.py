"""Replay of tests/golden/me_depth.npz (tests/golden/gen_me_depth_golden.py): the REAL InterSearch::xTZSearch and InterSearch::xMotionEstimation at 8 and 12 bits, on a
natural and a saturated scene, under the motion lambdas of QP 22 .. 63 at the depth -- the device against the recorded results without the reference, bit-exact."""
import json
import os

import numpy as np
import pytest

import me_util

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me_depth.npz")


def load(kind, bd, sat):
    """-> (scene, jobs, expected rows) of one recorded scene; fails when the scene generators no longer make the recorded pictures"""
    z = np.load(G)
    scenes = [tuple(int(v) for v in s) for s in z["scenes"]]
    scene = me_util.SaturatedScene(416, 240, bd, seed=60 + bd) if sat else me_util.DeepScene(416, 240, hard=True, bit_depth=bd)
    sums = [int(scene.cur.astype(np.int64).sum()), int(scene.ref_buf.astype(np.int64).sum())]
    assert sums == [int(v) for v in z["plane_sums"][scenes.index((bd, sat))]], "the scene generators changed: regenerate the golden file"
    jobs = [json.loads(str(s)) for s in z["%s_jobs_%d_%d" % (kind, bd, sat)]]
    for j in jobs:      # JSON has no tuples
        j["extra"] = [tuple(e) for e in j["extra"]]
        if "mvPred" in j:
            j["mvPred"], j["mv"] = tuple(j["mvPred"]), tuple(j["mv"])
    return scene, jobs, [tuple(int(v) for v in r) for r in z["%s_res_%d_%d" % (kind, bd, sat)]], tuple(int(v) for v in z["cfg"])


@pytest.mark.parametrize("sat", [0, 1])
@pytest.mark.parametrize("bd", [8, 12])
def test_tz_search_matches_reference_golden(ctx, bd, sat):
    from test_gpu_me import _run_hip
    scene, jobs, exp, _ = load("tz", bd, sat)
    assert len(jobs) >= 70
    got = [g[:4] for g in _run_hip(ctx, scene, jobs)]
    bad = [k for k in range(len(jobs)) if got[k] != exp[k]]
    assert not bad, [(jobs[k], got[k], exp[k]) for k in bad[:5]]


@pytest.mark.parametrize("sat", [0, 1])
@pytest.mark.parametrize("bd", [8, 12])
def test_motion_estimation_matches_reference_golden(ctx, bd, sat):
    from test_gpu_mest import run_device
    scene, jobs, exp, cfgv = load("mest", bd, sat)
    assert len(jobs) >= 70
    got, res = run_device(ctx, scene, jobs, cfgv)
    got = [g + ((0, 0) if j["bi"] else (r.intX, r.intY)) for g, j, r in zip(got, jobs, res)]
    bad = [k for k in range(len(jobs)) if got[k] != exp[k]]
    assert not bad, [(jobs[k], got[k], exp[k]) for k in bad[:5]]
