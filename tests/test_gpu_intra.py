"""GPU parity of the intra prediction entries: vtmhip_intra_pred_batch_dev (IntraPrediction::predIntraAng, PDPC included) and vtmhip_intra_presel_batch_dev (the
same prediction kept on chip and reduced to SAD and SATD against the original block) on their three launch paths (16, 64 and 256 lanes per job), at 8 / 10 / 12
bits and reference lines 0 .. 2 -- against the Python restatement of the reference (tests/intra_util.py, pinned to the real members in tests/test_intra.py and by
tests/golden/intra.npz), the oracle's distortions and vtmhip_dist_batch_dev.  Bit-exact.  The lines of every block lie between runs of 0x7fff longer than a line,
so parity also shows that nothing outside a block's own lines was read."""
import ctypes as C
import os

import numpy as np
import pytest

import intra_util as iu
from vtm_amd import lib
from vtm_amd.device import struct_array_to_numpy
from vtm_amd.lib import DistJob, VtmHipError

pytestmark = pytest.mark.gpu

# the smallest block without a filter (4x4), with one (8x8: planar; 16x4 / 4x16: none yet -- 64 samples but log2 size 3), the smallest PDPC (4x4); wide-angle size
# ratios 2, 4 and 16 in both orientations; every launch path
SHAPES = [(4, 4), (4, 8), (8, 4), (8, 8), (16, 4), (4, 16), (64, 4), (4, 64), (16, 16), (8, 32), (32, 32), (64, 64)]
PATHS = {16: [s for s in SHAPES if s[0] * s[1] <= 64], 64: [s for s in SHAPES if 64 < s[0] * s[1] <= 1024], 256: [s for s in SHAPES if s[0] * s[1] > 1024]}


def test_shape_list_reaches_every_launch_path():
    L = lib.load()
    assert {L.vtmhip_intra_lanes_per_job(w * h) for w, h in SHAPES} == {16, 64, 256}
    for lanes, shapes in PATHS.items():
        assert shapes and max(L.vtmhip_intra_lanes_per_job(w * h) for w, h in shapes) == lanes
    assert {abs(iu.flog2(w) - iu.flog2(h)) for w, h in SHAPES} >= {0, 1, 2, 4} and {w > h for w, h in SHAPES if w != h} == {True, False}


def _blocks(rng, shapes, bd, kind):
    return [iu.make_block(rng, w, h, m, bd, kind) for (w, h) in shapes for m in (0, 1, 2)]


@pytest.mark.parametrize("kind", ["random", "alt", "const"])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_prediction_parity(ctx, bd, kind):
    """all 67 modes on line 0 and modes 1 .. 66 on lines 1 and 2 of every shape, one call per launch path"""
    rng = np.random.default_rng(100 + bd)
    for lanes, shapes in PATHS.items():
        b = iu.Batch(_blocks(rng, shapes, bd, kind))
        assert b.n == len(shapes) * (67 + 66 + 66) and len(b.exp) == b.n
        if kind == "alt":     # where the projection of the side line breaks the alternation the cubic taps overshoot: the clip works at 0 and at the maximum
            assert min(p[0] for p in b.probe) < 0 and max(p[1] for p in b.probe) > (1 << bd) - 1
        b.check_pred(b.run_pred(ctx))


def test_golden_replay(ctx):
    """the recorded reference predictions, without the reference and without the restatement"""
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intra.npz")))
    blocks = []
    for w, h, m, bd, off in (tuple(int(v) for v in r) for r in g["blocks"]):
        nt, nl = 2 * w + 1 + m, 2 * h + 1 + m
        blocks.append(dict(w=w, h=h, m=m, bd=bd, top=g["lines"][off:off + nt], left=g["lines"][off + nt:off + nt + nl], modes=[]))
    for blk, mode in g["cases"][:, :2]:
        blocks[blk]["modes"].append(int(mode))
    b = iu.Batch(blocks)
    assert b.n == len(g["cases"]) and [(i, mode) for i, mode, _ in b.jobs] == [(int(r[0]), int(r[1])) for r in g["cases"]]
    assert [off for _, _, off in b.jobs] == [int(r[2]) for r in g["cases"]]
    assert np.array_equal(b.run_pred(ctx)[:b.pred_len], g["preds"])


@pytest.fixture(scope="module")
def fused():
    """one batch per launch path and a mixed one: every shape, the 35 first-round modes on line 0 and a handful on lines 1 / 2, bit depths rotating; the
    expectations are computed once"""
    rng, out = np.random.default_rng(77), {}
    for key, shapes in list(PATHS.items()) + [("mixed", SHAPES)]:
        blocks = []
        for k, (w, h) in enumerate(shapes):
            for m in (0, 1 + k % 2):
                blocks.append(iu.make_block(rng, w, h, m, (8, 10, 12)[(k + m) % 3], "random", iu.FIRST_ROUND if m == 0 else [1, 2, 19, 34, 50, 63]))
        plane = iu.place_in_plane(rng, blocks)
        b = iu.Batch(blocks)
        out[key] = (b, plane, b.exp_dist(plane))
    return out


@pytest.mark.parametrize("key", [16, 64, 256, "mixed"])
def test_fused_presel_against_the_oracle_and_the_two_step_route(ctx, fused, key):
    b, plane, exp = fused[key]
    assert all(blk["org_stride"] > blk["w"] for blk in b.blocks) and all(blk["org_off"] & 1 for blk in b.blocks)
    got = b.run_presel(ctx, plane)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:6].tolist()
    # the same numbers from vtmhip_dist_batch_dev on the predictions vtmhip_intra_pred_batch_dev wrote
    flat, bufs = b.run_pred(ctx, keep=True)
    b.check_pred(flat)
    dj = (DistJob * (2 * b.n))()
    for k, (i, mode, off) in enumerate(b.jobs):
        blk = b.blocks[i]
        for kind in (0, 1):
            dj[2 * k + kind] = DistJob(blk["org_off"], off, blk["org_stride"], blk["w"], blk["w"], blk["h"], 0, kind)
    d_org, d_dj, d_out = ctx.to_device(plane), ctx.to_device(struct_array_to_numpy(dj)), ctx.alloc(16 * b.n)
    ctx.dist_batch(d_org.ptr, bufs[3].ptr, d_dj.ptr, 2 * b.n, d_out.ptr)
    ctx.sync()
    assert np.array_equal(d_out.to_host(np.uint64).reshape(-1, 2), got)
    for buf in bufs + (d_org, d_dj, d_out):
        buf.free()


def test_batch_shapes(ctx, fused):
    rng = np.random.default_rng(9)
    # n = 1 on every path
    for w, h in ((4, 4), (16, 16), (64, 64)):
        blk = iu.make_block(rng, w, h, 0, 10, "random", [27])
        plane = iu.place_in_plane(rng, [blk])
        b = iu.Batch([blk])
        b.check_pred(b.run_pred(ctx))
        assert np.array_equal(b.run_presel(ctx, plane), b.exp_dist(plane))
    # one block with its 35 first-round modes, then 37 jobs: no multiple of 4, 8 or 16
    for w, h, modes in ((8, 8, iu.FIRST_ROUND), (16, 8, iu.FIRST_ROUND + [3, 5]), (64, 32, iu.FIRST_ROUND[:5])):
        blk = iu.make_block(rng, w, h, 0, 10, "random", modes)
        plane = iu.place_in_plane(rng, [blk])
        b = iu.Batch([blk])
        assert b.n == len(modes) and b.n % 4
        b.check_pred(b.run_pred(ctx))
        assert np.array_equal(b.run_presel(ctx, plane), b.exp_dist(plane))
    # a few hundred jobs of all shapes, bit depths and lines in one call, the jobs of a block scattered through the array
    mixed, plane, exp = fused["mixed"]
    assert mixed.n >= 300 and {blk["bd"] for blk in mixed.blocks} == {8, 10, 12} and {blk["m"] for blk in mixed.blocks} == {0, 1, 2}
    order = rng.permutation(mixed.n)
    s = iu.Batch(mixed.blocks, order=order)
    s._exp = [mixed.exp[k] for k in order]
    assert sum(s.jobs[k][0] != s.jobs[k + 1][0] for k in range(s.n - 1)) > s.n // 2   # scattered indeed
    s.check_pred(s.run_pred(ctx))
    assert np.array_equal(s.run_presel(ctx, plane), exp[order])


def test_malformed_jobs_are_skipped_and_arguments_checked(ctx):
    """mode 67, planar off line 0, a block index past the table, a block 128 wide: skipped, their outputs untouched (the fill pattern), the valid jobs exact"""
    rng = np.random.default_rng(13)
    blocks = [iu.make_block(rng, 8, 8, 0, 10, "random", [0, 1, 34, 66]), iu.make_block(rng, 16, 4, 1, 8, "random", [1, 2, 50]),
              iu.make_block(rng, 8, 8, 0, 10, "random", [18])]
    plane = iu.place_in_plane(rng, blocks)
    b = iu.Batch(blocks)
    assert b.n == 8
    bad = {1: ("mode", 67), 3: ("block", len(blocks)), 5: ("mode", 0), 7: ("width", 128)}   # job 5 sits on the line-1 block: planar with m = 1
    for k, (field, v) in bad.items():
        if field == "width":
            b.blk_arr[b.jobs[k][0]].width = v     # the third block has this job only
        else:
            setattr(b.job_arr[k], field, v)
    for k in (1, 5):
        assert b.jobs[k][0] == (0 if k == 1 else 1)
    flat = b.run_pred(ctx)
    b.check_pred(flat, skip=set(bad))
    fill16 = np.frombuffer(bytes([0xa5, 0xa5]), np.int16)[0]
    for k in bad:
        i, _, off = b.jobs[k]
        assert (flat[off:off + blocks[i]["w"] * blocks[i]["h"]] == fill16).all(), k
    got, exp = b.run_presel(ctx, plane), b.exp_dist(plane)
    for k in range(b.n):
        assert (got[k] == np.uint64(0xa5a5a5a5a5a5a5a5)).all() if k in bad else np.array_equal(got[k], exp[k]), k
    # host-side rejections: nothing is launched
    d = ctx.alloc(64)
    for args in ((None, d.ptr, 1, d.ptr, 1, d.ptr), (d.ptr, None, 1, d.ptr, 1, d.ptr), (d.ptr, d.ptr, 1, None, 1, d.ptr), (d.ptr, d.ptr, 1, d.ptr, 1, None),
                 (d.ptr, d.ptr, 1, d.ptr, -1, d.ptr), (d.ptr, d.ptr, 0, d.ptr, 1, d.ptr), (d.ptr, d.ptr, -1, d.ptr, 0, d.ptr)):
        with pytest.raises(VtmHipError):
            ctx.intra_pred_batch(*args)
    for args in ((None, d.ptr, d.ptr, 1, d.ptr, 1, d.ptr), (d.ptr, None, d.ptr, 1, d.ptr, 1, d.ptr), (d.ptr, d.ptr, d.ptr, 1, d.ptr, 1, None),
                 (d.ptr, d.ptr, d.ptr, 0, d.ptr, 1, d.ptr), (d.ptr, d.ptr, d.ptr, 1, d.ptr, -1, d.ptr)):
        with pytest.raises(VtmHipError):
            ctx.intra_presel_batch(*args)
    ctx.intra_pred_batch(None, None, 0, None, 0, None)
    ctx.intra_presel_batch(None, None, None, 0, None, 0, None)
    d.free()


def test_host_helper(ctx):
    """Context.intra_presel: numpy lines and mode lists in, predictions or (SAD, SATD) out"""
    rng = np.random.default_rng(21)
    blocks = [iu.make_block(rng, 8, 4, 0, 10, "random", [0, 2, 50]), iu.make_block(rng, 16, 16, 2, 10, "random", [1, 40])]
    plane = iu.place_in_plane(rng, blocks)
    b = iu.Batch(blocks)
    preds = ctx.intra_presel(blocks)
    assert len(preds) == 5 and all(np.array_equal(p, e) for p, e in zip(preds, b.exp))
    assert np.array_equal(ctx.intra_presel(blocks, plane), b.exp_dist(plane))
