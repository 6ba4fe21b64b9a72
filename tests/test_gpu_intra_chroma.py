"""GPU parity of the intra chroma entries: vtmhip_intra_chroma_pred_batch_dev (the regular modes of a chroma block, LM, MDLM_L, MDLM_T; Cb and Cr together) and
vtmhip_intra_chroma_presel_batch_dev (the same predictions kept on chip and reduced to SAD and SATD against the two originals) on both launch paths (16 and 64
lanes per job), at 8 / 10 / 12 bits -- against the Python restatement of the reference (tests/cclm_util.py, pinned in tests/test_cclm.py), the oracle's distortions
and vtmhip_dist_batch_dev.  Bit-exact.  The chroma lines lie between runs of 0x7fff and the luma planes hold 0x7fff wherever the host is not required to supply a
sample, so parity also shows that nothing outside a block's documented inputs was read."""
import numpy as np
import pytest

import cclm_util as cu
import oracle_lib as ol
from vtm_amd import lib
from vtm_amd.device import struct_array_to_numpy
from vtm_amd.lib import DistJob, VtmHipError

pytestmark = pytest.mark.gpu

# both lane widths (16: up to 64 samples, 64: up to 1024), wide angles on both sides (8x4 / 32x8 flat, 4x16 tall), the largest LDS footprint (32x32)
SHAPES = [(4, 4), (8, 4), (4, 16), (16, 16), (32, 8), (32, 32)]
STRIDE = 97
# regular modes at the rule boundaries of the chroma variant (fixed modes, integer and fractional slopes of both signs, the modes a wide angle moves) and the three LM modes
MODES = [0, 1, 2, 3, 7, 18, 19, 33, 34, 35, 49, 50, 51, 61, 65, 66] + cu.ALL_LM


def _avail(w, h, cls, k):
    """the class's availability, the above-right reach cut to what a plane of stride 97 holds"""
    above, left, ar, bl = cu.availability(cls, w, h, k)
    return above, left, min(ar, (STRIDE - 7) // 2 - w) & ~1, bl


def _blocks(rng, shapes, modes=MODES, kinds=("random", "alt", "const", "swing")):
    out, k = [], 0
    for w, h in shapes:
        for cls in cu.AVAIL_CLASSES:
            out.append(cu.make_block(rng, w, h, (8, 10, 12)[k % 3], kinds[k % len(kinds)], cls, coloc=(k + k // 6) % 2 == 1,
                                     first_row=(k % 6 // 2 + k // 12) % 2 == 1, modes=modes, stride=STRIDE,
                                     avail=_avail(w, h, cls, k)))
            k += 1
    return out


def _exp_dist(b, plane):
    out = np.zeros((b.n, 4), np.uint64)
    flat = plane.reshape(-1)
    for k, (i, mode, _) in enumerate(b.jobs):
        blk = b.blocks[i]
        for c in (0, 1):
            rows = blk["org_off"][c] + np.arange(blk["h"])[:, None] * blk["org_stride"] + np.arange(blk["w"])[None, :]
            org, pred = ol.i16(flat[rows]), ol.i16(b.exp[k][c])
            out[k, 2 * c], out[k, 2 * c + 1] = ol.o_dist(0, org, pred, blk["w"], blk["h"]), ol.o_dist(1, org, pred, blk["w"], blk["h"])
    return out


@pytest.fixture(scope="module")
def cases():
    """per launch path and mixed: every shape x availability class, bit depth / plane kind / collocated / first-row rotating; the expectations are computed once"""
    rng, out = np.random.default_rng(55), {}
    small, large = [s for s in SHAPES if s[0] * s[1] <= 64], [s for s in SHAPES if s[0] * s[1] > 64]
    for key, shapes in ((16, small), (64, large), ("mixed", SHAPES)):
        blocks = _blocks(rng, shapes, MODES if key != "mixed" else [1, 18, 50, 66] + cu.ALL_LM)
        plane = cu.place_orgs(rng, blocks)
        b = cu.Batch(blocks)
        out[key] = (b, plane)
    return out


def test_shape_list_reaches_both_lane_widths_and_ragged_luma():
    L = lib.load()
    assert {L.vtmhip_intra_lanes_per_job(w * h) for w, h in SHAPES} == {16, 64}
    rng = np.random.default_rng(1)
    blocks = _blocks(rng, SHAPES, [67])
    assert all(b["plane"].shape[1] == STRIDE and (b["lxy"][1] * STRIDE + b["lxy"][0]) & 1 for b in blocks)
    assert {(b["above"], b["left"]) for b in blocks} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(b["ar"] > b["h"] for b in blocks) and any(b["bl"] > b["w"] for b in blocks)       # the MDLM clamps
    assert any(0 < b["ar"] < b["w"] for b in blocks) and any(b["first_row"] for b in blocks) and any(b["coloc"] and not b["above"] for b in blocks)


@pytest.mark.parametrize("key", [16, 64])
def test_prediction_parity(ctx, cases, key):
    b, _ = cases[key]
    assert {blk["bd"] for blk in b.blocks} == {8, 10, 12}
    b.check_pred(b.run_pred(ctx))


def test_golden_replay(ctx):
    """the recorded reference predictions of every golden case (tests/golden/cclm.npz): the three LM modes and the recorded regular modes, without the reference"""
    import os
    cases = list(cu.golden_cases(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cclm.npz")))
    blocks = []
    for b, _, _, _, _, modes, _ in cases:
        b["modes"] = cu.ALL_LM + list(modes)
        blocks.append(b)
    batch = cu.Batch(blocks)
    batch._exp = [p for _, _, _, _, p_lm, _, p_rg in cases for p in list(p_lm) + list(p_rg)]
    assert batch.n == len(batch._exp) and batch.n > 1000
    batch.check_pred(batch.run_pred(ctx))


@pytest.mark.parametrize("key", [16, 64, "mixed"])
def test_fused_presel_against_the_oracle_and_the_two_step_route(ctx, cases, key):
    b, plane = cases[key]
    assert all(blk["org_off"][0] & 1 and blk["org_off"][1] & 1 for blk in b.blocks)
    got = b.run_presel(ctx, plane)
    exp = _exp_dist(b, plane)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:6].tolist()
    # the same numbers from vtmhip_dist_batch_dev on the predictions vtmhip_intra_chroma_pred_batch_dev wrote
    flat, bufs = b.run_pred(ctx, keep=True)
    b.check_pred(flat)
    dj = (DistJob * (4 * b.n))()
    for k, (i, mode, off) in enumerate(b.jobs):
        blk = b.blocks[i]
        for c in (0, 1):
            for kind in (0, 1):
                dj[4 * k + 2 * c + kind] = DistJob(blk["org_off"][c], off + c * blk["w"] * blk["h"], blk["org_stride"], blk["w"], blk["w"], blk["h"], 0, kind)
    d_org, d_dj, d_out = ctx.to_device(plane), ctx.to_device(struct_array_to_numpy(dj)), ctx.alloc(32 * b.n)
    ctx.dist_batch(d_org.ptr, bufs[4].ptr, d_dj.ptr, 4 * b.n, d_out.ptr)
    ctx.sync()
    assert np.array_equal(d_out.to_host(np.uint64).reshape(-1, 4), got)
    for buf in bufs + (d_org, d_dj, d_out):
        buf.free()


def test_batch_shapes(ctx, cases):
    rng = np.random.default_rng(9)
    # n = 1 on both paths, a regular and an LM mode
    for w, h in ((4, 4), (32, 32)):
        for mode in (27, cu.MDLM_T):
            blk = cu.make_block(rng, w, h, 10, "random", "full", modes=[mode], stride=STRIDE, avail=_avail(w, h, "full", 0))
            plane = cu.place_orgs(rng, [blk])
            b = cu.Batch([blk])
            assert b.n == 1
            b.check_pred(b.run_pred(ctx))
            assert np.array_equal(b.run_presel(ctx, plane), _exp_dist(b, plane))
    # 35 and 37 jobs of one block: no multiple of 8 or 16
    for (w, h), n in (((8, 4), 35), ((16, 16), 37), ((4, 16), 37)):
        modes = (list(range(0, 67, 2)) + cu.ALL_LM + [3])[:n]
        blk = cu.make_block(rng, w, h, 10, "random", "partial", coloc=True, modes=modes, stride=STRIDE, k=1, avail=_avail(w, h, "partial", 1))
        plane = cu.place_orgs(rng, [blk])
        b = cu.Batch([blk])
        assert b.n == n
        b.check_pred(b.run_pred(ctx))
        assert np.array_equal(b.run_presel(ctx, plane), _exp_dist(b, plane))
    # a shuffled job table: regular and LM modes of several blocks in one chunk
    mixed, plane = cases["mixed"]
    order = rng.permutation(mixed.n)
    s = cu.Batch(mixed.blocks, order=order)
    s._exp = [mixed.exp[k] for k in order]
    assert sum(s.jobs[k][0] != s.jobs[k + 1][0] for k in range(s.n - 1)) > s.n // 2
    chunks = [s.jobs[k:k + 8] for k in range(0, s.n, 8)]
    assert any(len({i for i, _, _ in c}) > 2 and {m >= cu.LM for _, m, _ in c} == {True, False} for c in chunks)
    s.check_pred(s.run_pred(ctx))
    assert np.array_equal(s.run_presel(ctx, plane), _exp_dist(mixed, plane)[order])


@pytest.mark.parametrize("shape", [(4, 4), (16, 16)])
def test_a_run_whose_only_lm_job_is_the_last_of_its_chunk(ctx, shape):
    """the down-sampled luma is staged for a run although its first jobs do not ask for it, and not for the runs before and after"""
    rng = np.random.default_rng(31)
    w, h = shape
    chunk = 16 if w * h <= 64 else 8
    regular = [1, 18, 50, 2, 34, 66, 10, 26, 42, 58, 3, 5, 7, 9, 11]
    blocks = [cu.make_block(rng, w, h, 10, "random", "full", modes=regular[:chunk - 1] + [cu.MDLM_L], stride=STRIDE, avail=_avail(w, h, "full", 0)),
              cu.make_block(rng, w, h, 8, "random", "both", coloc=True, modes=regular[:chunk - 1] + [cu.LM], stride=STRIDE),
              cu.make_block(rng, w, h, 12, "random", "left", modes=regular[:3], stride=STRIDE)]
    plane = cu.place_orgs(rng, blocks)
    b = cu.Batch(blocks)
    assert b.n == 2 * chunk + 3 and b.jobs[chunk - 1][1] == cu.MDLM_L and b.jobs[2 * chunk - 1][1] == cu.LM
    b.check_pred(b.run_pred(ctx))
    assert np.array_equal(b.run_presel(ctx, plane), _exp_dist(b, plane))


def test_malformed_jobs_and_blocks_are_skipped_and_arguments_checked(ctx):
    """mode 70, a block index past the table, and blocks with a side of 2 / 64, bit depth 13, above-right without above, an odd below-left count, below-left beyond
    the side, a flag of 2: skipped, their outputs untouched (the fill pattern); the valid jobs around them exact"""
    rng = np.random.default_rng(13)
    mk = lambda w, h, modes, cls="full": cu.make_block(rng, w, h, 10, "random", cls, modes=modes, stride=STRIDE, avail=_avail(w, h, cls, 0))   # noqa: E731
    blocks = [mk(8, 8, [0, 67, 34, 69])] + [mk(8, 8, [67, 1]) for _ in range(7)] + [mk(4, 4, [68, 50])]
    plane = cu.place_orgs(rng, blocks)
    b = cu.Batch(blocks)
    bad_blocks = {1: ("width", 2), 2: ("height", 64), 3: ("bitDepth", 13), 4: ("above", 0), 5: ("belowLeft", 3), 6: ("belowLeft", 10), 7: ("firstRow", 2)}
    for i, (field, v) in bad_blocks.items():
        setattr(b.blk_arr[i], field, v)
    assert blocks[4]["ar"] > 0
    b.job_arr[1].mode = 70
    b.job_arr[3].block = len(blocks)
    bad = {1, 3} | {k for k, (i, _, _) in enumerate(b.jobs) if i in bad_blocks}
    assert len(bad) == 16 and b.n == 20
    flat = b.run_pred(ctx)
    b.check_pred(flat, skip=bad)
    fill16 = np.frombuffer(bytes([0xa5, 0xa5]), np.int16)[0]
    for k in bad:
        i, _, off = b.jobs[k]
        assert (flat[off:off + 2 * blocks[i]["w"] * blocks[i]["h"]] == fill16).all(), k
    got, exp = b.run_presel(ctx, plane), _exp_dist(b, plane)
    for k in range(b.n):
        assert (got[k] == np.uint64(0xa5a5a5a5a5a5a5a5)).all() if k in bad else np.array_equal(got[k], exp[k]), k
    # host-side rejections: nothing is launched
    d = ctx.alloc(64).ptr
    for args in ((None, d, d, 1, d, 1, d), (d, None, d, 1, d, 1, d), (d, d, None, 1, d, 1, d), (d, d, d, 1, None, 1, d), (d, d, d, 1, d, 1, None),
                 (d, d, d, 1, d, -1, d), (d, d, d, 0, d, 1, d), (d, d, d, -1, d, 0, d)):
        with pytest.raises(VtmHipError) as e:
            ctx.intra_chroma_pred_batch(*args)
        assert e.value.status == lib.E_INVALID
    for args in ((None, d, d, d, 1, d, 1, d), (d, None, d, d, 1, d, 1, d), (d, d, None, d, 1, d, 1, d), (d, d, d, None, 1, d, 1, d), (d, d, d, d, 1, None, 1, d),
                 (d, d, d, d, 1, d, 1, None), (d, d, d, d, 0, d, 1, d), (d, d, d, d, 1, d, -1, d)):
        with pytest.raises(VtmHipError) as e:
            ctx.intra_chroma_presel_batch(*args)
        assert e.value.status == lib.E_INVALID
    ctx.intra_chroma_pred_batch(None, None, None, 0, None, 0, None)
    ctx.intra_chroma_presel_batch(None, None, None, None, 0, None, 0, None)


def test_host_helper(ctx):
    """Context.intra_chroma_presel: numpy lines, a luma array and mode lists in, predictions or the four distortions out"""
    rng = np.random.default_rng(21)
    blocks = [cu.make_block(rng, 8, 4, 10, "random", "full", modes=[0, 2, 68]), cu.make_block(rng, 16, 16, 8, "swing", "above", coloc=True, modes=[67, 40, 69], k=1)]
    plane = cu.place_orgs(rng, blocks)
    b = cu.Batch(blocks)
    preds = ctx.intra_chroma_presel(blocks, b.luma_buf)
    assert len(preds) == 6 and all(np.array_equal(p, e) for p, e in zip(preds, b.exp))
    assert np.array_equal(ctx.intra_chroma_presel(blocks, b.luma_buf, plane), _exp_dist(b, plane))
