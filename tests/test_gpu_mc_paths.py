"""vtmhip_motion_compensation_batch_dev and vtmhip_xEstimateMvPredAMVP_batch_dev on each of their four launch forms (vtmhip_mc_lanes_per_block of the hint: 8 or 16 lanes
per block with eight / four blocks in a wave, a wave per block, a workgroup per block), bit-exact against the oracle at 8, 10 and 12 bits.  The prediction tables
(tests/mc_util.py) put blocks of different filters side by side in a wave and lay their outputs out with odd strides and offsets in buffers compared as a whole."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import mc_util
import me_util
import oracle_lib as ol
from test_gpu_mest import _scene, hip_jobs
from vtm_amd import lib
from vtm_amd.lib import MeJob, PicParams, VtmHipError

gpu = pytest.mark.gpu

HINTS = {8: [(8, 8), (16, 4), (4, 16)], 16: [(16, 16), (32, 8), (8, 32)], 64: [(32, 32), (64, 16), (16, 64)], 256: [(64, 32), (32, 64)]}
DEPTHS = [8, 10, 12]


def lanes_of(hint):
    return lib.load().vtmhip_mc_lanes_per_block(*hint)


# ---- no device ------------------------------------------------------------------------------------------------------------------------
def test_hints_reach_every_path():
    assert set(HINTS) == {8, 16, 64, 256}
    for lanes, hints in HINTS.items():
        assert hints and all(lanes_of(h) == lanes for h in hints), lanes
        for h in hints:      # every table has blocks of the hint's own size; all but the 4-wide hint have blocks of both filters
            shapes = mc_util.shapes_in_hint(h)
            assert (h[0], h[1], 0) in shapes and {w % 8 == 0 for w, _, _ in shapes} == ({True, False} if h[0] >= 8 else {False}), (h, shapes)


def test_path_rule_boundaries():
    """vtmhip_mc_lanes_per_block: 8 lanes up to 64 samples, 16 up to 256, a wave up to 1024, the workgroup above; 0 for a side outside 2 .. 128"""
    f = lib.load().vtmhip_mc_lanes_per_block
    assert [f(8, 8), f(13, 5)] == [8, 16]                                  # 64 / 65 samples
    assert [f(16, 16), f(128, 2), f(2, 128), f(3, 86), f(86, 3)] == [16, 16, 16, 64, 64]      # 256 / 258 (257 is prime: no block has it)
    assert [f(32, 32), f(128, 8), f(41, 25), f(128, 128)] == [64, 64, 256, 256]      # 1024 / 1025
    assert [f(2, 2), f(1, 8), f(8, 1), f(129, 2), f(2, 129), f(0, 0), f(-4, -4)] == [8, 0, 0, 0, 0, 0, 0]
    for w in range(2, 129):
        for h in range(2, 129):
            a = w * h
            assert f(w, h) == (8 if a <= 64 else 16 if a <= 256 else 64 if a <= 1024 else 256), (w, h)


def test_batch_sizes_leave_partial_waves_and_an_xcd_remainder():
    for lanes in HINTS:
        jpb = mc_util.jobs_per_wave(lanes)
        sizes = mc_util.batch_sizes(lanes)
        assert sizes[0] == 1 and (jpb == 1 or jpb - 1 in sizes)
        n = sizes[-1]
        assert n <= 200 and (jpb == 1 or n % jpb) and -(-n // jpb) % 8 not in (0, 1), (lanes, n)


# sha256 of the job table, and the first 16 digits of those of the expected predictions and epilogue outputs, as the test's inline code made them
LEGACY_TABLES = {8: ("801d2530c607c2ff4c4bfe38cca6332d41fcb9f094480115aadeb0e84e8cd902", "d451a5b1bbec3606", "5c6fa5fa8bac0532"),
                 10: ("cba4458b8003af345004458aa0810a29bdfc3a961d9de713ced3a987e636a856", "d94a317a4a12e783", "28e6717edbc3ed90"),
                 12: ("06b6bdf743db954566db27ddb0609c1d1011225e282b3d33889b874646d8e98e", "b60c299efe3628f9", "9d40f26389058f3a")}


@pytest.mark.parametrize("bd", DEPTHS)
def test_table_of_the_fused_test_is_what_it_was(bd):
    """test_gpu_bipred.test_motion_compensation_fused_matches_oracle takes its jobs from mc_util.legacy_table: the table is byte for byte the one the test built inline
    before (digests taken from that code), so the move changed nothing of what the test runs."""
    _, jobs, exp_pred, exp_out, meta, pos = mc_util.legacy_table(bd)
    sha = lambda b: hashlib.sha256(b).hexdigest()      # noqa: E731
    assert sha(bytes(jobs)) == LEGACY_TABLES[bd][0]
    assert (sha(np.concatenate(exp_pred).tobytes())[:16], sha(np.concatenate(exp_out).tobytes())[:16]) == LEGACY_TABLES[bd][1:]
    assert len(jobs) == (500 if bd == 10 else 250) and pos == sum(e.size for e in exp_pred) == sum(e.size for e in exp_out)


@pytest.mark.parametrize("lanes", [8, 16])
@pytest.mark.parametrize("bd", DEPTHS)
def test_waves_mix_filters_and_phases(lanes, bd):
    """From the job tables alone: at least half of the waves (jobs [k * JPB, (k + 1) * JPB)) of the path's large tables hold both block filters and at least three ways
    through them -- of every hint's table but the 4-wide one's, where no block has a width of 8 -- and over a table every (filter, phase) pair its luma shapes allow,
    both planes, every mode, epilogue and BCW weight occur."""
    jpb = mc_util.jobs_per_wave(lanes)
    all_mixed = all_waves = 0
    for hi, hint in enumerate(HINTS[lanes]):
        t = mc_util.path_table(hint, bd, _seed(lanes, bd, hi), mc_util.batch_sizes(lanes)[-1])
        waves = [t.jobs[k:k + jpb] for k in range(0, t.n, jpb)]
        mixed = sum(1 for w in waves if len({mc_util.width_class(j) for j in w}) >= 2 and len({mc_util.phase_class(j) for j in w}) >= 3)
        assert 2 * mixed >= len(waves) or hint[0] < 8, (hint, mixed, len(waves))
        assert 2 * sum(1 for w in waves if len({mc_util.phase_class(j) for j in w}) >= 3) >= len(waves)
        all_mixed, all_waves = all_mixed + mixed, all_waves + len(waves)
        jobs = list(t.jobs)
        luma_filters = {"vec" if w % 8 == 0 else "scalar" for w, _, c in mc_util.shapes_in_hint(hint) if not c}
        assert {(mc_util.width_class(j), mc_util.phase_class(j)) for j in jobs if not j.chroma} >= {(w, p) for w in luma_filters for p in mc_util.PHASES}, hint
        assert {j.chroma for j in jobs} == {0, 1} and {j.mode for j in jobs} == {0, 1, 2} and {j.epilogue for j in jobs} == {0, 1, 2}
        assert {j.bcwWeight for j in jobs if j.epilogue == 2} == {0, 4, -2, 3, 5, 10}
        assert all(j.width <= hint[0] and j.height <= hint[1] and j.predStride > j.width and j.outStride > j.width and j.predOff != j.outOff for j in jobs)
        assert all((j.predStride - j.width) % 2 and (j.outStride - j.width) % 2 for j in jobs)
        for odd in (sum(j.predOff & 1 for j in jobs), sum(j.outOff & 1 for j in jobs)):
            assert t.n // 4 <= odd <= 3 * t.n // 4
    assert 2 * all_mixed >= all_waves


def _seed(lanes, bd, hint_index):
    return 4000 + 100 * lanes + 10 * bd + hint_index


# ---- motion compensation --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("lanes", [8, 16, 64, 256])
def test_motion_compensation_on_each_path(ctx, lanes, bd):
    """Every hint of the path at n = 1, JPB - 1 and the large n; per table three calls (both outputs, prediction only, epilogue output only).  The WHOLE output buffers
    are compared: a sample outside its block, or of a job without an epilogue, must still be the fill."""
    pic = mc_util.pictures(bd)
    d_org, d_ref = ctx.to_device(pic.orgs), ctx.to_device(pic.refs)
    for hi, hint in enumerate(HINTS[lanes]):
        assert lanes_of(hint) == lanes
        for n in mc_util.batch_sizes(lanes):
            t = mc_util.path_table(hint, bd, _seed(lanes, bd, hi), n)
            assert all(j.width <= hint[0] and j.height <= hint[1] for j in t.jobs)      # (a larger block is the caller's error: the kernel does not guard it)
            d_jobs = ctx.to_device(np.frombuffer(t.jobs, np.uint8))
            for want_pred, want_out in ((1, 1), (1, 0), (0, 1)):
                d_pred = ctx.to_device(np.full(t.exp_pred.size, mc_util.FILL, np.int16))
                d_out = ctx.to_device(np.full(t.exp_out.size, mc_util.FILL, np.int16))
                ctx.motion_compensation_batch(d_org.ptr, d_ref.ptr, d_pred.ptr if want_pred else None, d_out.ptr if want_out else None, d_jobs.ptr, n, hint[0], hint[1])
                gp, go = d_pred.to_host(np.int16), d_out.to_host(np.int16)
                for name, got, exp, want in (("pred", gp, t.exp_pred, want_pred), ("out", go, t.exp_out, want_out)):
                    if not want:
                        assert np.all(got == mc_util.FILL), (name, "written though not asked for", hint, n, bd)
                        continue
                    bad = np.flatnonzero(got != exp)
                    assert bad.size == 0, (name, hint, n, bd, (want_pred, want_out), _where(t, name, int(bad[0])), int(got[bad[0]]), int(exp[bad[0]]), bad.size)
                for b in (d_pred, d_out):
                    b.free()
            d_jobs.free()


def _where(t, name, at):
    """(job, row, column) of the first wrong sample, or the job whose block it follows"""
    for k, (pp, ps, po, os_, cw, ch) in enumerate(t.blocks):
        o, s = (pp, ps) if name == "pred" else (po, os_)
        if o <= at < o + ch * s:
            j = t.jobs[k]
            return dict(job=k, y=(at - o) // s, x=(at - o) % s, w=cw, h=ch, chroma=j.chroma, mode=j.mode, epi=j.epilogue, bcw=j.bcwWeight, phase=mc_util.phase_class(j))
    return dict(offset=at, outside="every block")


# ---- AMVP estimation ------------------------------------------------------------------------------------------------------------------
def _sides(v):
    return [s for s in (4, 8, 16, 32, 64) if s <= v]


def _limits(scene, j):
    """clipMvInPic's range of a row's vector (Mv.cpp:56-74), for the coverage floors only"""
    return ((-128 - 8 - j["x"] + 1) << 4, (scene.W + 8 - j["x"] - 1) << 4, (-128 - 8 - j["y"] + 1) << 4, (scene.H + 8 - j["y"] - 1) << 4)


def _row(scene, w, h, x, y, cands, imv=0, num=2, idx_bits=(1, 1), lam=20.0, bits=5):
    return dict(w=w, h=h, x=x, y=y, bi=0, imv=imv, mvpIdx=0, numCand=num, cands=[list(c) for c in cands], mvPred=tuple(cands[0]), mv=(0, 0), idxBits=tuple(idx_bits), bits=bits,
                searchRange=64, lam=lam, extra=[], other_seed=0)


FLAT = (288, 16, 96, 96)      # x, y, width, height of the patch painted flat into the reference picture


def _amvp_rows(scene, hint, bd, seed):
    """(rows, number of generated rows): ~150 rows of the search tests' generator on the sides that fit the hint, then the hand-made ones at the hint's size"""
    w, h = hint
    lams = me_util.real_lambdas(bd)
    rows = me_util.random_mest_jobs(scene, 150, seed=seed, sizes=(_sides(w), _sides(h)), lams=lams)
    n_gen = len(rows)
    far = 9000                                                     # 562 samples: beyond clipMvInPic's range from anywhere in the picture
    rows.append(_row(scene, w, h, 64, 64, [(-37 * 16 + 5, 29 * 16 + 3), (0, 0)], num=1, lam=lams[0]))      # one candidate: the (better) second entry is not looked at
    rows.append(_row(scene, w, h, 128, 96, [(35, -18), (35, -18)], lam=lams[1]))                            # equal candidates: index 0
    fx, fy = FLAT[0] + 16, FLAT[1] + 16                            # a block of up to 64 x 64, displaced by up to 6 samples, with its filter taps: inside the patch
    rows.append(_row(scene, w, h, fx, fy, [(-16 * 4 + 3, 16 * 2 + 7), (16 * 3 + 9, -16 * 5 + 1)], lam=lams[2]))      # both predictions inside the flat patch: a cost tie
    rows.append(_row(scene, w, h, fx, fy, [(16 * 6, 0), (-16 * 2 + 8, 16 * 3 + 8)], imv=3, lam=lams[2]))             # the same with the alternative half-pel taps
    for cx, cy in ((0, 0), (scene.W - w, 0), (0, scene.H - h), (scene.W - w, scene.H - h)):
        for sx, sy in ((-1, -1), (1, 1), (-1, 1), (1, -1)):        # both candidates far outside, in opposite directions; then one of them near
            rows.append(_row(scene, w, h, cx, cy, [(sx * far, sy * far), (-sx * far, -sy * far)], lam=lams[(cx + cy + sx) % 5], idx_bits=(1, 2)))
        rows.append(_row(scene, w, h, cx, cy, [(far, -far), (16, -12)], lam=lams[3], idx_bits=(2, 1)))
    for k, (a, b) in enumerate(((3, -2), (-7, 4), (0, 0), (12, 9))):      # imv 3 at fraction 8 in both components: the alternative half-pel filter in H and V
        rows.append(_row(scene, w, h, 96 + 32 * k, 48 + 24 * k, [(16 * a + 8, 16 * b + 8), (16 * b + 8, 16 * a - 8)], imv=3, lam=lams[k], idx_bits=(1 + k % 2, 2 - k % 2)))
    return rows, n_gen


def _amvp_expect(scene, rows):
    L = ol.oracle()
    exp = []
    for j in rows:
        keep = []
        t = me_util.oracle_mest_job(scene, j, keep)
        a = [C.c_int(), C.c_int(), C.c_int(), C.c_uint64()]
        L.vo_estimate_mvp_amvp(C.byref(t), *[C.byref(x) for x in a])
        exp.append(tuple(x.value for x in a))      # (mvpIdx, mvPredHor, mvPredVer, distBiP)
    return exp


def _amvp_call(ctx, scene, bufs, rows, exp, hint, uniform, add_bits, with_dist, tag):
    """One call; compares the five results of every row and every other byte of the rows."""
    n = len(rows)
    arr = hip_jobs(scene, rows, np.zeros(1, np.int16))
    want = (MeJob * n).from_buffer_copy(bytes(arr))
    for k, (idx, ph, pv, _) in enumerate(exp):
        want[k].mvpIdx, want[k].mvPredHor, want[k].mvPredVer = idx, ph, pv
        want[k].bits = rows[k]["bits"] + (rows[k]["idxBits"][idx] if add_bits else 0)
    d_jobs = ctx.to_device(np.frombuffer(arr, np.uint8))
    d_dist = ctx.to_device(np.full(n + 2, 0xa5a5a5a5a5a5a5a5, np.uint64))
    pic = PicParams(scene.W, scene.H, 128, bd_of(scene), 0)
    ctx.estimate_mvp_amvp_batch(pic, bufs[0].ptr, bufs[1].ptr, d_jobs.ptr, n, hint[0], hint[1], uniform=uniform, add_idx_bits=add_bits, d_dist_bip=d_dist.ptr if with_dist else None)
    got = (MeJob * n).from_buffer_copy(d_jobs.to_host(np.uint8).tobytes())
    dist = d_dist.to_host(np.uint64)
    for k in range(n):
        g, e = got[k], want[k]
        assert (g.mvpIdx, g.mvPredHor, g.mvPredVer, g.bits) == (e.mvpIdx, e.mvPredHor, e.mvPredVer, e.bits), (tag, hint, k, rows[k], exp[k])
        assert bytes(g) == bytes(e), (tag, hint, k, "a byte outside mvpIdx / mvPred / bits changed")
    if with_dist:
        assert [int(v) for v in dist[:n]] == [e[3] for e in exp], (tag, hint)
        assert np.all(dist[n:] == np.uint64(0xa5a5a5a5a5a5a5a5))
    else:
        assert np.all(dist == np.uint64(0xa5a5a5a5a5a5a5a5))
    d_jobs.free()
    d_dist.free()
    return [(g.mvpIdx, g.mvPredHor, g.mvPredVer, g.bits) for g in got]


def bd_of(scene):
    return getattr(scene, "bd", 10)


def _flat_scene(bd):
    """The search tests' picture pair with a patch of the reference painted mid-grey: every prediction inside it is the same block"""
    scene = _scene(bd)
    x, y, w, h = FLAT
    m = scene.margin
    scene.ref_buf.reshape(-1, scene.ref_stride)[m + y:m + y + h, m + x:m + x + w] = 1 << (bd - 1)
    return scene


def _cand_costs(scene, j):
    """template cost of each candidate alone (the oracle on one-candidate copies of the row)"""
    return [_amvp_expect(scene, [dict(j, numCand=1, cands=[j["cands"][c], j["cands"][c]], idxBits=(j["idxBits"][c],) * 2)])[0][3] for c in (0, 1)]


@gpu
@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("lanes", [8, 16, 64, 256])
def test_amvp_estimation_on_each_path(ctx, lanes, bd):
    """vtmhip_xEstimateMvPredAMVP_batch_dev = vo_estimate_mvp_amvp per row (itself pinned to InterSearch::xEstimateMvPredAMVP in test_oracle_vs_ref.py): the winner, the
    UNCLIPPED winning candidate, the bits with and without the index bits, the winning cost with and without its buffer; a table of rows of the hint's size gives the same
    under uniformSize.  The floors below are taken from the expected values only."""
    scene = _flat_scene(bd)
    bufs = (ctx.to_device(scene.cur), ctx.to_device(scene.ref_buf))
    wins, clipped, ties = [0, 0], [0, 0, 0, 0], 0
    for hi, hint in enumerate(HINTS[lanes]):
        assert lanes_of(hint) == lanes
        rows, n_gen = _amvp_rows(scene, hint, bd, 6000 + 100 * lanes + 10 * bd + hi)
        for j in rows:
            j["bi"] = 0
        assert all(j["w"] <= hint[0] and j["h"] <= hint[1] for j in rows) and len(rows) <= 200
        exp = _amvp_expect(scene, rows)
        for k, j in enumerate(rows):
            if k < n_gen and j["numCand"] == 2:
                wins[exp[k][0]] += 1
            lo_h, hi_h, lo_v, hi_v = _limits(scene, j)
            for c in j["cands"][:j["numCand"]]:
                for d, out in enumerate((c[0] < lo_h, c[0] > hi_h, c[1] < lo_v, c[1] > hi_v)):
                    clipped[d] += out
            if j["numCand"] == 2 and j["cands"][0] != j["cands"][1] and j["idxBits"][0] == j["idxBits"][1]:
                a, b = _cand_costs(scene, j)
                if a == b:
                    ties += 1
                    assert exp[k][0] == 0
            if j["cands"][0] == j["cands"][1] and j["idxBits"][0] <= j["idxBits"][1]:
                assert exp[k][0] == 0
        for add_bits in (0, 1):
            for with_dist in (0, 1):
                _amvp_call(ctx, scene, bufs, rows, exp, hint, 0, add_bits, with_dist, ("mixed", add_bits, with_dist))
        same = [k for k, j in enumerate(rows) if (j["w"], j["h"]) == hint]
        assert len(same) >= 25
        a = _amvp_call(ctx, scene, bufs, [rows[k] for k in same], [exp[k] for k in same], hint, 0, 1, 1, "one size")
        b = _amvp_call(ctx, scene, bufs, [rows[k] for k in same], [exp[k] for k in same], hint, 1, 1, 1, "one size, uniformSize")
        assert a == b
    assert min(wins) >= 0.3 * sum(wins) and sum(wins) >= 200, wins
    assert min(clipped) >= 1 and ties >= 1, (clipped, ties)
    for b in bufs:
        b.free()


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
@gpu
def test_calls_with_nothing_to_do_and_bad_hints(ctx):
    """n == 0 is a call that does nothing; a hint side outside 2 .. 128 (AMVP: 4 .. 128), an epilogue output without the original plane and a NULL table are refused,
    and a refused call has written nothing."""
    t = mc_util.path_table((8, 8), 10, 77, 7)
    pic = t.pic
    d_org, d_ref, d_jobs = ctx.to_device(pic.orgs), ctx.to_device(pic.refs), ctx.to_device(np.frombuffer(t.jobs, np.uint8))
    d_pred, d_out = ctx.to_device(np.full(t.exp_pred.size, mc_util.FILL, np.int16)), ctx.to_device(np.full(t.exp_out.size, mc_util.FILL, np.int16))
    ctx.motion_compensation_batch(d_org.ptr, d_ref.ptr, d_pred.ptr, d_out.ptr, d_jobs.ptr, 0, 8, 8)
    for args in ((d_org.ptr, d_ref.ptr, d_pred.ptr, d_out.ptr, d_jobs.ptr, 7, 1, 8), (d_org.ptr, d_ref.ptr, d_pred.ptr, d_out.ptr, d_jobs.ptr, 7, 8, 1),
                 (d_org.ptr, d_ref.ptr, d_pred.ptr, d_out.ptr, d_jobs.ptr, 7, 129, 8), (d_org.ptr, d_ref.ptr, d_pred.ptr, d_out.ptr, d_jobs.ptr, 7, 8, 129),
                 (None, d_ref.ptr, d_pred.ptr, d_out.ptr, d_jobs.ptr, 7, 8, 8),      # an epilogue output without the original plane
                 (d_org.ptr, d_ref.ptr, d_pred.ptr, d_out.ptr, None, 7, 8, 8),       # no job table
                 (d_org.ptr, d_ref.ptr, None, None, d_jobs.ptr, 7, 8, 8),            # nothing to write
                 (d_org.ptr, d_ref.ptr, d_pred.ptr, d_out.ptr, d_jobs.ptr, -1, 8, 8)):
        with pytest.raises(VtmHipError):
            ctx.motion_compensation_batch(*args)
    assert np.all(d_pred.to_host(np.int16) == mc_util.FILL) and np.all(d_out.to_host(np.int16) == mc_util.FILL)

    scene = _scene(10)
    rows = me_util.random_mest_jobs(scene, 5, seed=1, sizes=([8], [8]))
    for j in rows:
        j["bi"] = 0
    arr = hip_jobs(scene, rows, np.zeros(1, np.int16))
    c_org, c_ref, d_rows = ctx.to_device(scene.cur), ctx.to_device(scene.ref_buf), ctx.to_device(np.frombuffer(arr, np.uint8))
    d_dist = ctx.to_device(np.full(5, 0xa5a5a5a5a5a5a5a5, np.uint64))
    p = PicParams(scene.W, scene.H, 128, 10, 0)
    ctx.estimate_mvp_amvp_batch(p, c_org.ptr, c_ref.ptr, d_rows.ptr, 0, 8, 8, d_dist_bip=d_dist.ptr)
    for args in ((p, c_org.ptr, c_ref.ptr, d_rows.ptr, 5, 1, 8), (p, c_org.ptr, c_ref.ptr, d_rows.ptr, 5, 8, 1), (p, c_org.ptr, c_ref.ptr, d_rows.ptr, 5, 129, 8),
                 (p, c_org.ptr, c_ref.ptr, d_rows.ptr, 5, 8, 129), (p, c_org.ptr, c_ref.ptr, None, 5, 8, 8), (p, None, c_ref.ptr, d_rows.ptr, 5, 8, 8)):
        with pytest.raises(VtmHipError):
            ctx.estimate_mvp_amvp_batch(*args, d_dist_bip=d_dist.ptr)
    assert np.all(d_dist.to_host(np.uint64) == np.uint64(0xa5a5a5a5a5a5a5a5)) and d_rows.to_host(np.uint8).tobytes() == bytes(arr)
    for b in (d_org, d_ref, d_jobs, d_pred, d_out, c_org, c_ref, d_rows, d_dist):
        b.free()
