"""GPU parity: the Hadamard distortion of the affine search (block_dist of affine.hip) on every launch form and lane layout.

The estimation kernel runs one wave per job when the launch bounds hold at most 1024 samples and four waves above; on <= 10-bit pictures a group of eight lanes
shares one 8x8 Hadamard unit when the job has at most a quarter as many units as lanes, and a lane takes a whole unit otherwise.  tests/test_gpu_affine.py always
launches with bounds 128 x 128, so this file launches one batch per block shape with the bounds of that shape.  Expected values: the oracle
(vo_affine_motion_estimation), bit-exact, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import me_util
import oracle_lib as ol
from test_gpu_affine import hip_jobs, oracle_results
from vtm_amd.lib import AffineMeOut, PicParams

pytestmark = pytest.mark.gpu

ONE_WAVE = [(16, 16), (32, 16), (16, 32), (32, 32), (64, 16), (16, 64)]        # bounds <= 1024 samples: 64 threads
FOUR_WAVES_GROUPS = [(64, 32), (32, 64), (64, 64), (128, 16), (16, 128)]       # 256 threads, eight lanes per unit
FOUR_WAVES_UNITS = [(128, 64), (128, 128)]                                     # 256 threads, a lane per unit
SHAPES = ONE_WAVE + FOUR_WAVES_GROUPS + FOUR_WAVES_UNITS
EDGE_SHAPES = [(16, 16), (32, 16), (32, 32), (64, 64)]

_scenes, _expected = {}, {}


def scene_of(kind):
    if kind not in _scenes:
        _scenes[kind] = {"hard10": lambda: me_util.Scene(416, 240, hard=True),
                         "deep8": lambda: me_util.DeepScene(416, 240, hard=True, bit_depth=8),
                         "sat10": lambda: me_util.SaturatedScene(416, 240, bit_depth=10),
                         "sat10_signed": lambda: me_util.SaturatedScene(416, 240, bit_depth=10, signed=True)}[kind]()
    return _scenes[kind]


def has_mix(jobs):
    return any(j["bi"] for j in jobs) and any(j["six"] for j in jobs) and any(not j["six"] for j in jobs)


def draw_jobs(scene, shapes, n, seed, bd, all_bi=False):
    """About n jobs of the wanted shapes, Hadamard distortion on all of them; more are taken from the same draw until a bi job and both models are among them."""
    sizes = tuple(sorted({s for wh in shapes for s in wh}))
    pool = [j for j in me_util.random_affine_jobs(scene, 16 * n * len(sizes) ** 2, seed, sizes=sizes if len(sizes) > 1 else sizes * 2, bit_depth=bd) if (j["w"], j["h"]) in shapes]
    for j in pool:
        j["satd"] = 1
        if all_bi:
            j["bi"] = 1
    jobs = pool[:n]
    for j in pool[n:]:
        if has_mix(jobs):
            break
        jobs.append(j)
    assert len(jobs) >= n and has_mix(jobs), (len(jobs), shapes)
    return jobs


def expected(kind, shapes, n, seed, bd, all_bi=False):
    """(jobs, oracle results, hevc costs, start-model predictions) of a batch: computed once per batch and shared."""
    key = (kind, tuple(shapes), n, seed, all_bi)
    if key not in _expected:
        scene = scene_of(kind)
        jobs = draw_jobs(scene, shapes, n, seed, bd, all_bi)
        _expected[key] = (jobs,) + oracle_results(scene, jobs, ol.oracle(), bd)
    return _expected[key]


def run_device(ctx, scene, jobs, hevc, bd, max_w, max_h):
    others = np.zeros(max(1, sum(j["w"] * j["h"] for j in jobs if j["bi"])), np.int16)
    arr, _ = hip_jobs(scene, jobs, others, hevc)
    pic = PicParams(scene.W, scene.H, 128, bd, 0)
    d_cur, d_ref, d_oth = ctx.to_device(scene.cur), ctx.to_device(scene.ref_buf), ctx.to_device(others)
    d_jobs = ctx.to_device(np.frombuffer(arr, np.uint8))
    d_res = ctx.alloc(C.sizeof(AffineMeOut) * len(jobs))
    ctx.affine_motion_estimation_batch(pic, d_cur.ptr, d_ref.ptr, d_oth.ptr, d_jobs.ptr, len(jobs), max_w, max_h, d_res.ptr)
    res = (AffineMeOut * len(jobs)).from_buffer_copy(d_res.to_host(np.uint8).tobytes())
    return [([tuple(v) for v in r.mv][:3 if j["six"] else 2], r.bits, r.cost, r.iterations, r.refinements) for r, j in zip(res, jobs)]


def check(ctx, kind, shapes, n, seed, bd, max_w, max_h, all_bi=False):
    jobs, exp, hevc, preds = expected(kind, shapes, n, seed, bd, all_bi)
    got = run_device(ctx, scene_of(kind), jobs, hevc, bd, max_w, max_h)
    for k, j in enumerate(jobs):
        assert got[k] == exp[k], ("xAffineMotionEstimation", (max_w, max_h), k, j, got[k], exp[k])
    assert sum(e[3] for e in exp) > 0 and sum(e[4] for e in exp) > len(jobs)      # gradient steps and refinement steps were evaluated
    return jobs, preds


@pytest.mark.parametrize("kind,bd", [("hard10", 10), ("deep8", 8)])
@pytest.mark.parametrize("w,h", SHAPES)
def test_affine_me_shape_with_its_own_launch_bounds(ctx, w, h, kind, bd):
    """One batch per block shape, launched with maxWidth x maxHeight = that shape: both launch forms, grouped and one-lane units, square / 16x8 / 8x16 tiles.
    4- and 6-parameter, uni and bi, the three AMVR precisions, PROF on and off come from the generator."""
    n = 12 if w * h >= 128 * 64 else 24      # the oracle's large blocks dominate the test's time
    check(ctx, kind, [(w, h)], n, 100 + w + 3 * h, bd, w, h)


@pytest.mark.parametrize("kind,bd", [("hard10", 10), ("deep8", 8)])
def test_affine_me_mixed_shapes_in_one_wave_launch(ctx, kind, bd):
    """16x16 and 32x32 jobs in one batch with bounds 32 x 32: the lane layout follows the job, not the launch bounds."""
    jobs, _ = check(ctx, kind, [(16, 16), (32, 32)], 32, 7, bd, 32, 32)
    assert {(j["w"], j["h"]) for j in jobs} == {(16, 16), (32, 32)}


def largest_difference(scene, jobs, preds):
    """per job: max |pattern - prediction of the start model|, pattern = 2 * org - other (from the expected side alone)"""
    out = []
    for j, p in zip(jobs, preds):
        org = scene.cur.reshape(scene.H, scene.W)[j["y"]:j["y"] + j["h"], j["x"]:j["x"] + j["w"]].astype(np.int64)
        pat = 2 * org - me_util.other_pred(scene, j).astype(np.int64)
        out.append(int(np.abs(pat - p.astype(np.int64)).max()))
    return out


@pytest.mark.parametrize("w,h", EDGE_SHAPES)
def test_affine_me_bi_on_saturated_picture(ctx, w, h):
    """All jobs bi on the saturated 10-bit picture pair.  Samples in 0 .. 1023 bound the pattern 2 * org - other by -1023 .. 2046 and so |pattern - prediction| by
    2046: no plain 10-bit picture goes beyond 2047; the batch must come close to that bound."""
    jobs, preds = check(ctx, "sat10", [(w, h)], 24, 300 + w + 3 * h, 10, w, h, all_bi=True)
    assert max(largest_difference(scene_of("sat10"), jobs, preds)) >= 2040


@pytest.mark.parametrize("w,h", EDGE_SHAPES)
def test_affine_me_bi_beyond_three_packed_levels(ctx, w, h):
    """The same on the saturated pair whose original is itself a bi-pred target (2 * org - other, up to 2046): the pattern reaches 4092 and |pattern - prediction|
    exceeds 2047 (asserted from the expected side), still inside the +-4095 the packed Hadamard is entered for.  16 * 2048 leaves int16: a fourth butterfly level in
    packed 16-bit words would have overflowed."""
    jobs, preds = check(ctx, "sat10_signed", [(w, h)], 24, 300 + w + 3 * h, 10, w, h, all_bi=True)
    big = largest_difference(scene_of("sat10_signed"), jobs, preds)
    assert max(big) > 2047 and max(big) <= 4095, max(big)
