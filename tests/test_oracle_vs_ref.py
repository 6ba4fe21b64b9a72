"""CPU, dev container only: the plain-C oracle against the REAL reference (oracle/_ref/libvtmref.so, built from
/root/reference by oracle/Makefile.ref) on randomized sweeps -- wider than the committed golden fixtures.
Skipped where the reference build is absent (e.g. a fresh checkout on the GPU box before `make -f oracle/Makefile.ref`)."""
import ctypes as C

import numpy as np
import pytest

import me_util
import oracle_lib as ol

pytestmark = pytest.mark.ref


def test_distortion_sweep(oracle, reflib):
    rng = np.random.default_rng(101)
    for w in (4, 8, 12, 16, 24, 32, 48, 64, 128):
        for h in (4, 8, 16, 32, 64, 128):
            for _ in range(2):
                org = ol.i16(rng.integers(-1023, 2047, (h, w + 7)))
                cur = ol.i16(rng.integers(0, 1024, (h, w + 3)))
                for ss in (0, 1):
                    assert ol.o_dist(0, org, cur, w, h, ss) == ol.r_dist(0, 1, org, cur, w, h, 10, ss) == ol.r_dist(0, 0, org, cur, w, h, 10, ss)
                assert ol.o_dist(1, org, cur, w, h) == ol.r_dist(1, 1, org, cur, w, h) == ol.r_dist(1, 0, org, cur, w, h)
                assert ol.o_dist(2, org, cur, w, h) == ol.r_dist(2, 0, org, cur, w, h)
            for mode in (0, 1, 2, 3):
                assert oracle.vo_subshift_for_mode(w, h, mode) == reflib.ref_subshift_for_mode(w, h, mode)
    # chroma / small shapes (2-wide blocks, 2x2 Hadamard tiles) as the encoder's own calls have them
    for (w, h) in ((2, 2), (2, 4), (2, 8), (2, 32), (4, 2), (8, 2), (16, 2), (64, 2)):
        org = ol.i16(rng.integers(0, 1024, (h, w + 7)))
        cur = ol.i16(rng.integers(0, 1024, (h, w + 3)))
        assert ol.o_dist(0, org, cur, w, h, 0) == ol.r_dist(0, 1, org, cur, w, h, 10, 0)
        assert ol.o_dist(1, org, cur, w, h) == ol.r_dist(1, 1, org, cur, w, h)
        assert ol.o_dist(2, org, cur, w, h) == ol.r_dist(2, 1, org, cur, w, h)


def test_satd8_grid_matches_reference_distfunc(oracle, reflib):
    scene = me_util.Scene(128, 64, hard=True, margin=16)
    nb, r = (128 // 8) * (64 // 8), 4
    a, b = np.zeros(nb * 81, np.uint64), np.zeros(nb * 81, np.uint64)
    refp = C.c_void_p(scene.ref_buf.ctypes.data + 2 * scene.ref_off)
    oracle.vo_satd8_grid(ol.P(scene.cur), 128, refp, scene.ref_stride, 128, 64, r, ol.P(a))
    reflib.ref_satd8_grid(1, ol.P(scene.cur), 128, refp, scene.ref_stride, 128, 64, r, 10, ol.P(b))
    assert np.array_equal(a, b)


def test_tap_tables_and_matrices(oracle, reflib):
    for which, name, nf, nt in ((0, "vo_luma_filter", 16, 8), (1, "vo_luma_filter_4x4", 16, 8), (2, "vo_chroma_filter", 32, 4)):
        tab = np.array((C.c_int16 * (nf * nt)).in_dll(oracle, name)).reshape(nf, nt)
        for f in range(nf):
            o = np.zeros(8, np.int16)
            reflib.ref_if_taps(which, f, ol.P(o))
            assert np.array_equal(o[:nt], tab[f])
    alt = np.zeros(8, np.int16)
    reflib.ref_if_taps(4, 0, ol.P(alt))
    assert np.array_equal(alt, np.array((C.c_int16 * 8).in_dll(oracle, "vo_luma_alt_hpel")))
    for t in range(3):
        for n in (2, 4, 8, 16, 32, 64):
            a, b = np.zeros((n, n), np.int16), np.zeros((n, n), np.int16)
            ra, rb = oracle.vo_tr_matrix(t, n, ol.P(a)), reflib.ref_tr_matrix(t, n, 0, ol.P(b))
            assert (ra == 0) == (rb == 0)
            if ra == 0:
                assert np.array_equal(a, b)
                reflib.ref_tr_matrix(t, n, 1, ol.P(b))   # the "inverse" table is the same matrix; the inverse transform indexes it transposed
                assert np.array_equal(a, b)


def test_interpolation_sweep(oracle, reflib):
    """8-, 10- and 12-bit; the 12-bit sources draw from their own generator (the 8- and 10-bit draws are unchanged) and put a third of their
    samples at 0 or 2^bd - 1, so the first-pass sums reach their extremes."""
    rng, rng12 = np.random.default_rng(102), np.random.default_rng(112)
    for (w, h) in ((4, 4), (4, 11), (4, 8), (8, 8), (16, 16), (17, 24), (5, 12), (64, 72), (12, 16)):
        for bd in (8, 10, 12):
            r = rng12 if bd == 12 else rng
            src = ol.i16(r.integers(0, 1 << bd, (h + 16, w + 16)))
            src14 = ol.i16(r.integers(-8192, 8191, (h + 16, w + 16)))
            if bd == 12:
                ext = r.random(src.shape) < 0.33
                src[ext] = r.integers(0, 2, int(ext.sum())) * ((1 << bd) - 1)
            ss = w + 16
            off = 8 * ss + 8
            for comp, nfr in ((0, 16), (1, 32)):
                for frac in range(nfr):
                    for isLast in (0, 1):
                        d = [np.zeros((h, w + 5), np.int16) for _ in range(3)]
                        oracle.vo_if_hor(comp, C.c_void_p(src.ctypes.data + 2 * off), ss, ol.P(d[0]), w + 5, w, h, frac, isLast, bd, 0, 0, 0)
                        for simd in (0, 1):
                            reflib.ref_if_hor(simd, comp, C.c_void_p(src.ctypes.data + 2 * off), ss, ol.P(d[1 + simd]), w + 5, w, h, frac, isLast,
                                              bd, 0, 0, 0)
                        assert np.array_equal(d[0], d[1]) and np.array_equal(d[0], d[2]), ("hor", w, h, bd, comp, frac, isLast)
                        for isFirst in (0, 1):
                            s = src if isFirst else src14
                            oracle.vo_if_ver(comp, C.c_void_p(s.ctypes.data + 2 * off), ss, ol.P(d[0]), w + 5, w, h, frac, isFirst, isLast, bd, 0,
                                             0, 0)
                            for simd in (0, 1):
                                reflib.ref_if_ver(simd, comp, C.c_void_p(s.ctypes.data + 2 * off), ss, ol.P(d[1 + simd]), w + 5, w, h, frac,
                                                  isFirst, isLast, bd, 0, 0, 0)
                            assert np.array_equal(d[0], d[1]) and np.array_equal(d[0], d[2]), ("ver", w, h, bd, comp, frac, isFirst, isLast)


def test_transform_1d_sweep(oracle, reflib):
    """All table slots with the skip combinations xT / xIT can produce; amplitudes up to 2^20 wrap in 32 bits on both sides.
    (Other skip values are not comparable: the small DCT-2 butterflies ignore iSkipLine2, TrQuant_EMT.cpp:51-232.)"""
    rng = np.random.default_rng(103)
    for t in range(3):
        for n in (2, 4, 8, 16, 32, 64):
            si = int(np.log2(n)) - 1
            sk2s = {0, 16 if (t != 0 and n == 32) else (n - 32 if n > 32 else 0)}
            for line in (1, 2, 4, 8, 16, 32, 64):
                for sk1 in {0} | ({16} if line == 32 else set()) | ({32} if line == 64 else set()):
                    for sk2 in sk2s:
                        for amp, shift in ((512, 1), (32767, 7), (1 << 20, 12)):
                            src = rng.integers(-amp, amp, line * n).astype(np.int32)
                            d1, d2 = np.full(line * n, -7, np.int32), np.full(line * n, -7, np.int32)
                            ra = oracle.vo_fwd_trans(t, n, ol.P(src), ol.P(d1), shift, line, sk1, sk2)
                            rb = reflib.ref_fwd_trans(t, si, ol.P(src), ol.P(d2), shift, line, sk1, sk2)
                            assert ra == rb and (ra != 0 or np.array_equal(d1, d2)), ("fwd", t, n, line, sk1, sk2)
                            s2 = src.reshape(n, line).copy()
                            if sk2:
                                s2[n - sk2:, :] = 0
                            if sk1:
                                s2[:, line - sk1:] = 0
                            ra = oracle.vo_inv_trans(t, n, ol.P(s2), ol.P(d1), shift, line, sk1, sk2, -32768, 32767)
                            rb = reflib.ref_inv_trans(t, si, ol.P(s2), ol.P(d2), shift, line, sk1, sk2, -32768, 32767)
                            assert ra == rb and (ra != 0 or np.array_equal(d1, d2)), ("inv", t, n, line, sk1, sk2)


@pytest.mark.parametrize("hard", [True, False])
def test_tz_search_equals_reference_xTZSearch(oracle, reflib, hard):
    scene = me_util.Scene(416, 240, hard=hard)
    jobs = me_util.random_tz_jobs(scene, 600, seed=201 + hard)
    exp = []
    for j in jobs:
        org = np.ascontiguousarray(scene.cur[j["y"]:j["y"] + j["h"], j["x"]:j["x"] + j["w"]])
        c, t, r = me_util.oracle_ctx(scene, j, org), me_util.oracle_tz_job(j), ol.MeResult()
        reflib.ref_tz_search(C.byref(c), C.byref(t), C.byref(r))
        exp.append((r.mvX, r.mvY, r.cost, r.dist))
    got = [g[:4] for g in me_util.run_oracle_tz(scene, jobs)]
    assert got == exp


def test_frac_and_full_search_equal_reference(oracle, reflib):
    scene = me_util.Scene(416, 240, hard=True)
    rng = np.random.default_rng(203)
    for trial in range(250):
        w = int(rng.choice([8, 16, 32, 64, 128, 4, 16, 8, 32, 64]))
        h = int(rng.choice([8, 16, 32, 64, 128, 8, 4, 16]))
        if w == 4 and h == 4:
            continue
        x = int(rng.integers(0, (416 - w) // 4 + 1)) * 4
        y = int(rng.integers(0, (240 - h) // 4 + 1)) * 4
        org = np.ascontiguousarray(scene.cur[y:y + h, x:x + w])
        if trial % 3 == 0:   # bi-pred ME target
            org = (2 * org.astype(np.int32) - rng.integers(0, 1024, org.shape)).astype(np.int16)
        j = dict(w=w, h=h, x=x, y=y, subShift=0, lam=float(rng.uniform(1, 40)), predHor=int(rng.integers(-64, 64)), predVer=int(rng.integers(-64, 64)))
        c = me_util.oracle_ctx(scene, j, org)
        ix, iy, had = int(rng.integers(-12, 12)), int(rng.integers(-12, 12)), int(trial % 4 != 0)
        a, b = ol.FracResult(), ol.FracResult()
        oracle.vo_frac_search(C.byref(c), ix, iy, had, 0, C.byref(a))
        reflib.ref_frac_search(C.byref(c), ix, iy, had, 0, C.byref(b))
        assert (a.halfX, a.halfY, a.qterX, a.qterY, a.cost) == (b.halfX, b.halfY, b.qterX, b.qterY, b.cost)
        sr, out = ol.Range(), (C.c_int * 4)()
        oracle.vo_set_search_range(C.byref(c), ix * 16, iy * 16, 4, C.byref(sr))
        reflib.ref_set_search_range(C.byref(c), ix * 16, iy * 16, 4, out)
        assert list(out) == [sr.left, sr.right, sr.top, sr.bottom]
        c.subShift = 1 if (h > 8 and w <= 64) else 0
        m, r = ol.MeResult(), ol.MeResult()
        oracle.vo_full_search(C.byref(c), C.byref(sr), C.byref(m))
        reflib.ref_full_search(C.byref(c), out, C.byref(r))
        assert (m.mvX, m.mvY, m.cost, m.dist) == (r.mvX, r.mvY, r.cost, r.dist)


def test_quant_dequant_equal_reference(oracle, reflib):
    """The real Quant::quant / Quant::dequant (flat scaling list, no SBH) through a minimal TransformUnit rig."""
    rng = np.random.default_rng(204)
    for w in (4, 8, 16, 32, 64):
        for h in (4, 8, 16, 32, 64):
            for qp in (22, 27, 32, 37, 45, 51):
                for irap in (0, 1):
                    c = rng.integers(-32768, 32768, w * h).astype(np.int32)
                    c[rng.random(w * h) < 0.5] //= 64
                    c2 = c.reshape(h, w)   # inputs respect the transform's zero-out (the reference's scan loop reads past its table otherwise)
                    c2[32:, :] = 0
                    c2[:, 32:] = 0
                    q1, d1, q2, d2 = (np.zeros(w * h, np.int32) for _ in range(4))
                    s1, s2 = C.c_int32(), C.c_int32()
                    reflib.ref_quant_dequant(ol.P(c), w, h, 10, qp, irap, ol.P(q1), C.byref(s1), ol.P(d1))
                    bq = qp + 12
                    oracle.vo_quant(ol.P(c), w, h, 10, bq // 6, bq % 6, irap, 0, ol.P(q2), None, C.byref(s2))
                    oracle.vo_dequant(ol.P(q2), w, h, 10, bq // 6, bq % 6, 0, ol.P(d2))
                    assert np.array_equal(q1, q2) and np.array_equal(d1, d2) and s1.value == s2.value, (w, h, qp, irap)


def quant_extreme_coefs(rng, w, h, amp=32768):
    """Coefficients for Quant::quant: random, a quarter of them at the int16 limits (the lowest QPs turn those into levels at the int16 limits, which
    is what dequant then sees), zeroed outside the transform's 32 x 32 zero-out."""
    c = rng.integers(-amp, amp, w * h).astype(np.int32)
    c[rng.random(w * h) < 0.4] //= 64
    ext = rng.random(w * h) < 0.25
    c[ext] = np.where(rng.random(int(ext.sum())) < 0.5, -amp, amp - 1)
    c2 = c.reshape(h, w)
    c2[32:, :] = 0
    c2[:, 32:] = 0
    return c


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_quant_dequant_full_qp_range_equal_reference(oracle, reflib, bd):
    """Quant::quant / dequant at every QP of the depth (-6 (bd - 8) .. 63, so qpPer from 0 to 14 at 12 bits), every TU size, plain and transform skip.
    The transform shift 15 - bd - log2 size is negative for 64-sample sides at 10 bits and from 32 x 32 on at 12; the dequant right shift goes negative at
    high qpPer (the left-shift-and-clip path).  The job's qpPer / qpRem come from the caller: for transform skip the reference's QpParam raises the
    base QP to at least 4 (QP' = 4 + 6 * internalMinusInputBitDepth), which matters below QP 4 - 6 (bd - 8); the test maps QP the same way."""
    rng = np.random.default_rng(205 + bd)
    off = 6 * (bd - 8)
    sizes = [(w, h) for w in (4, 8, 16, 32, 64) for h in (4, 8, 16, 32, 64)]
    qmax = dmax = dmin = 0
    for qp in range(-off, 64):
        for i, (w, h) in enumerate(sizes):
            for ts in (0, 1):
                if ts and max(w, h) > 32:
                    continue
                irap = (qp + i + ts) & 1
                c = quant_extreme_coefs(rng, w, h) if not ts else rng.integers(-(1 << bd) + 1, 1 << bd, w * h).astype(np.int32)
                if ts:
                    c[rng.random(w * h) < 0.25] = (1 << bd) - 1
                q1, d1, q2, d2 = (np.zeros(w * h, np.int32) for _ in range(4))
                s1, s2 = C.c_int32(), C.c_int32()
                reflib.ref_quant_dequant2(ol.P(c), w, h, bd, qp, irap, ts, ol.P(q1), C.byref(s1), ol.P(d1))
                bq = max(qp + off, 4) if ts else qp + off   # QpParam: the transform-skip QP' is at least 4 (Quant.cpp:93-98)
                oracle.vo_quant(ol.P(c), w, h, bd, bq // 6, bq % 6, irap, ts, ol.P(q2), None, C.byref(s2))
                oracle.vo_dequant(ol.P(q2), w, h, bd, bq // 6, bq % 6, ts, ol.P(d2))
                assert np.array_equal(q1, q2) and np.array_equal(d1, d2) and s1.value == s2.value, (w, h, qp, irap, ts, bd)
                qmax, dmax, dmin = max(qmax, int(np.abs(q1).max())), max(dmax, int(d1.max())), min(dmin, int(d1.min()))
    # the extremes were reached: dequantised values clipped to the int16 limits (high QPs); at 12 bits also levels clipped to them (lowest QPs)
    assert dmax == 32767 and dmin == -32768 and (bd < 12 or qmax == 32768), (qmax, dmax, dmin)


@pytest.mark.parametrize("use_had,fen,ext,first_stop", [(1, 1, 0, 1), (0, 1, 0, 0), (1, 0, 1, 1)])
def test_motion_estimation_equals_reference_xMotionEstimation(oracle, reflib, use_had, fen, ext, first_stop):
    """Whole InterSearch::xMotionEstimation (uni TZ / bi exhaustive, fractional refinement or AMVR integer refinement, final rate
    re-weighting) on a rig around the real member function vs the oracle's composition."""
    scene = me_util.Scene(416, 240, hard=True)
    cfg = ol.MestCfg(4, use_had, fen, ext, first_stop)
    jobs = me_util.random_mest_jobs(scene, 160, seed=300 + use_had * 4 + fen * 2 + ext)
    seen = set()
    for j in jobs:
        keep = []
        t = me_util.oracle_mest_job(scene, j, keep)
        a, b = ol.MestResult(), ol.MestResult()
        oracle.vo_motion_estimation(C.byref(cfg), C.byref(t), C.byref(a))
        reflib.ref_motion_estimation(C.byref(cfg), C.byref(t), C.byref(b))
        assert a.key() == b.key(), (j, a.key(), b.key())
        if not j["bi"]:
            assert (a.intX, a.intY) == (b.intX, b.intY)
        seen.add((j["bi"], j["imv"]))
    assert len(seen) == 8   # uni / bi x the four AMVR modes


@pytest.mark.parametrize("weight", [-2, 3, 5, 10])
def test_motion_estimation_bi_under_a_bcw_weight_equals_reference(oracle, reflib, weight):
    """The bi refinement of xMotionEstimation under a CU-level BCW weight (cu.BcwIdx != BCW_DEFAULT, InterSearch.cpp:3320-3328, 3483, 7666-7676): the search target is
    removeWeightHighFreq( org, otherPred, w ) and the distortion weight |w| / 8 -- the real member on the rig vs the oracle, the four AMVR modes."""
    scene = me_util.Scene(416, 240, hard=True)
    cfg = ol.MestCfg(4, 1, 1, 0, 1)
    jobs = [j for j in me_util.random_mest_jobs(scene, 420, seed=900 + weight) if j["bi"]]
    seen = set()
    for j in jobs:
        j["bcw"] = weight
        keep = []
        t = me_util.oracle_mest_job(scene, j, keep)
        a, b = ol.MestResult(), ol.MestResult()
        oracle.vo_motion_estimation(C.byref(cfg), C.byref(t), C.byref(a))
        reflib.ref_motion_estimation(C.byref(cfg), C.byref(t), C.byref(b))
        assert a.key() == b.key(), (j, a.key(), b.key())
        seen.add(j["imv"])
    assert len(jobs) >= 60 and len(seen) == 4


def test_pred_inter_blk_luma_and_chroma(oracle, reflib, bd=10):
    """InterPrediction::xPredInterBlk on a rig (real member function, Picture aliasing our planes) vs vo_mc_block: luma 8-tap / chroma
    4-tap at 1/32 phase, uni (rounded, clipped) and bi (14-bit intermediates), alternative half-sample filter; 8-, 10- and 12-bit pictures
    (me_util.to_bit_depth: the 12-bit one has flat areas at 0 and 4095)."""
    from vtm_amd import synth
    W, H, m = 416, 240, 64
    y, u, v = (me_util.to_bit_depth(p, bd) for p in synth.gen_frames(W, H, 1, chroma=True)[0])
    yb, yo, ys = synth.extend_plane(y, m)
    ub, uo, us = synth.extend_plane(u, m // 2)
    rng = np.random.default_rng(77 if bd == 10 else 77 + bd)
    for t in range(500 if bd == 10 else 250):
        w = int(rng.choice([4, 8, 16, 32, 64, 128]))
        h = int(rng.choice([4, 8, 16, 32, 64, 128]))
        if w > W or h > H or (w == 4 and h == 4):
            continue
        x = int(rng.integers(0, (W - w) // 4 + 1)) * 4
        yy = int(rng.integers(0, (H - h) // 4 + 1)) * 4
        mvh, mvv = int(rng.integers(-20 * 16, 20 * 16)), int(rng.integers(-20 * 16, 20 * 16))
        if t % 5 == 0:
            mvh &= ~15
        if t % 7 == 0:
            mvv &= ~15
        if t % 11 == 0:
            mvh = (mvh & ~15) | 8
        bi, imv, comp = int(t % 2), 3 if t % 3 == 0 else 0, int(t % 3 != 1) and (1 + t % 2) or 0
        cw, ch = (w // 2, h // 2) if comp else (w, h)
        a, b = np.zeros((ch, cw), np.int16), np.zeros((ch, cw), np.int16)
        if comp:
            refp = ub.ctypes.data + 2 * (uo + (yy // 2) * us + x // 2)
            oracle.vo_mc_block(comp, C.c_void_p(refp), us, cw, ch, mvh, mvv, bi, bd, int(imv == 3), ol.P(a), cw)
        else:
            refp = yb.ctypes.data + 2 * (yo + yy * ys + x)
            oracle.vo_mc_block(0, C.c_void_p(refp), ys, cw, ch, mvh, mvv, bi, bd, int(imv == 3), ol.P(a), cw)
        reflib.ref_pred_inter_blk(comp, C.c_void_p(yb.ctypes.data + 2 * yo), ys, C.c_void_p(ub.ctypes.data + 2 * uo), us, W, H, x, yy, w, h, mvh, mvv,
                                  bi, bd, imv, ol.P(b), cw)
        assert np.array_equal(a, b), (t, comp, w, h, mvh, mvv, bi, imv, bd)


def _masked_cases(rng, n):
    """(org, cur, w, h, mask array, mask_off, maskStride, stepX, maskStride2) in the caller's convention of EncCu.cpp:2930-2960:
    a 112x112 weight plane, rows walked with +-maskStride, columns with stepX, maskStride2 = -stepX * width."""
    M = 112
    plane = ol.i16(rng.integers(0, 9, (M, M)))
    out = []
    for k in range(n):
        w, h = int(rng.choice([8, 16, 32, 64])), int(rng.choice([8, 16, 32, 64]))
        org, cur = ol.i16(rng.integers(0, 1024, (h, w + 5))), ol.i16(rng.integers(0, 1024, (h, w + 3)))
        step_x = 1 if k % 3 else -1
        row_dir = 1 if k % 2 else -1
        x0 = int(rng.integers(0, M - w)) + (w - 1 if step_x < 0 else 0)
        y0 = int(rng.integers(0, M - h)) + (h - 1 if row_dir < 0 else 0)
        out.append((org, cur, w, h, plane.reshape(-1), y0 * M + x0, row_dir * M, step_x, -step_x * w))
    return out


def test_masked_sad_equals_reference(oracle, reflib):
    oracle.vo_sad_mask.restype = C.c_uint64
    reflib.ref_sad_mask.restype = C.c_uint64
    rng = np.random.default_rng(404)
    for org, cur, w, h, mask, off, ms, sx, ms2 in _masked_cases(rng, 300):
        mp = C.c_void_p(mask.ctypes.data + 2 * off)
        a = oracle.vo_sad_mask(ol.P(org), org.shape[1], ol.P(cur), cur.shape[1], w, h, 0, mp, ms, sx, ms2)
        b = reflib.ref_sad_mask(1, ol.P(org), org.shape[1], ol.P(cur), cur.shape[1], w, h, 10, mp, ms, sx, ms2)
        c = reflib.ref_sad_mask(0, ol.P(org), org.shape[1], ol.P(cur), cur.shape[1], w, h, 10, mp, ms, sx, ms2)
        assert a == b == c, (w, h, ms, sx, ms2)


def test_geo_blend_equals_reference(oracle, reflib):
    """vo_weighted_geo_blk vs InterpolationFilter::xWeightedGeoBlk (scalar) and the x86 m_weightedGeoBlk entry: every split direction, luma and
    4:2:0 chroma, 8- and 10-bit; the walk comes from the reference's own GEO tables (ref_geo_walk)."""
    M = 112
    planes = np.zeros((6, M, M), np.int16)
    for i in range(6):
        reflib.ref_geo_weights(i, ol.P(planes[i]))
    assert planes.min() == 0 and planes.max() == 8
    rng = np.random.default_rng(910)
    for split in range(64):
        for k in range(6):
            lw, lh = int(rng.choice([8, 16, 32, 64])), int(rng.choice([8, 16, 32, 64]))
            comp, bd = k % 3, (8 if k == 5 else 10)
            w, h = (lw >> 1, lh >> 1) if comp else (lw, lh)
            s0 = ol.i16(rng.integers(-8192, 8192 + 1023 * 16, (h, w + 3)))
            s1 = ol.i16(rng.integers(-8192, 8192 + 1023 * 16, (h, w + 5)))
            walk = (C.c_int * 4)()
            reflib.ref_geo_walk(split, comp, lw, lh, walk)
            mi, off, sx, ws = list(walk)
            a, b, c = (np.zeros((h, w), np.int16) for _ in range(3))
            reflib.ref_weighted_geo_blk(0, split, comp, lw, lh, ol.P(s0), w + 3, ol.P(s1), w + 5, ol.P(a), w, bd)
            reflib.ref_weighted_geo_blk(1, split, comp, lw, lh, ol.P(s0), w + 3, ol.P(s1), w + 5, ol.P(b), w, bd)
            oracle.vo_weighted_geo_blk(ol.P(s0), w + 3, ol.P(s1), w + 5, ol.P(c), w, w, h, C.c_void_p(planes[mi].ctypes.data + 2 * off), sx, ws, bd, 0,
                                       (1 << bd) - 1)
            assert np.array_equal(a, b) and np.array_equal(a, c), (split, comp, lw, lh, bd)
    # 12-bit: own generator; 14-bit intermediates over the whole range a 12-bit prediction produces (-8192 .. 8192 + 4095 * 4) and at its two ends
    rng, bd, lo, top = np.random.default_rng(912), 12, 1 << 12, 0
    hi = 8192 + ((1 << bd) - 1) * (1 << (14 - bd))
    for split in range(64):
        for comp in range(3):
            lw, lh = int(rng.choice([8, 16, 32, 64])), int(rng.choice([8, 16, 32, 64]))
            w, h = (lw >> 1, lh >> 1) if comp else (lw, lh)
            s0, s1 = ol.i16(rng.integers(-8192, hi + 1, (h, w + 3))), ol.i16(rng.integers(-8192, hi + 1, (h, w + 5)))
            s0[:, ::3], s1[:, 1::3] = hi, -8192
            walk = (C.c_int * 4)()
            reflib.ref_geo_walk(split, comp, lw, lh, walk)
            mi, off, sx, ws = list(walk)
            a, b, c = (np.zeros((h, w), np.int16) for _ in range(3))
            reflib.ref_weighted_geo_blk(0, split, comp, lw, lh, ol.P(s0), w + 3, ol.P(s1), w + 5, ol.P(a), w, bd)
            reflib.ref_weighted_geo_blk(1, split, comp, lw, lh, ol.P(s0), w + 3, ol.P(s1), w + 5, ol.P(b), w, bd)
            oracle.vo_weighted_geo_blk(ol.P(s0), w + 3, ol.P(s1), w + 5, ol.P(c), w, w, h, C.c_void_p(planes[mi].ctypes.data + 2 * off), sx, ws, bd, 0,
                                       (1 << bd) - 1)
            assert np.array_equal(a, b) and np.array_equal(a, c), (split, comp, lw, lh, bd)
            lo, top = min(lo, int(a.min())), max(top, int(a.max()))
    assert lo == 0 and top == (1 << bd) - 1


def test_bdof_equals_reference(oracle, reflib):
    """vo_bdof_pu vs the reference's xPredInterBlk(bioApplied) + applyBiOptFlow, with the scalar and with the x86 buffer ops; the refinement must
    actually move samples (differs from the plain bi-prediction average on this content)."""
    from vtm_amd import synth
    W, H, M = 192, 128, 48
    fr = list(synth.gen_frames(W, H, 3, seed=5))
    p0, p1 = (np.ascontiguousarray(np.pad(f.astype(np.int16), M, mode="edge")) for f in (fr[0], fr[2]))
    S = p0.shape[1]

    def at(p, x, y):
        return C.c_void_p(p.ctypes.data + 2 * ((y + M) * S + x + M))
    rng = np.random.default_rng(1011)
    moved = 0
    for k in range(120):
        w, h = int(rng.choice([8, 16, 32, 64, 128])), int(rng.choice([8, 16, 32, 64, 128]))
        if w * h < 128:
            continue
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        mv = [int(v) for v in rng.integers(-500, 500, 4)]
        if k % 6 == 0:
            mv[k % 4] &= ~15
        bd = 8 if k % 10 == 9 else 10
        q0, q1 = (p0 >> 2, p1 >> 2) if bd == 8 else (p0, p1)
        q0, q1 = np.ascontiguousarray(q0), np.ascontiguousarray(q1)
        a, b, c, avg = (np.zeros((h, w), np.int16) for _ in range(4))
        reflib.ref_bdof_pu(0, at(q0, 0, 0), at(q1, 0, 0), S, W, H, x, y, w, h, *mv, bd, ol.P(a), w)
        reflib.ref_bdof_pu(1, at(q0, 0, 0), at(q1, 0, 0), S, W, H, x, y, w, h, *mv, bd, ol.P(b), w)
        oracle.vo_bdof_pu(at(q0, x, y), S, at(q1, x, y), S, w, h, *mv, bd, ol.P(c), w)
        assert np.array_equal(a, b) and np.array_equal(a, c), (k, x, y, w, h, mv, bd)
        t0, t1 = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
        oracle.vo_mc_block(0, at(q0, x, y), S, w, h, mv[0], mv[1], 1, bd, 0, ol.P(t0), w)
        oracle.vo_mc_block(0, at(q1, x, y), S, w, h, mv[2], mv[3], 1, bd, 0, ol.P(t1), w)
        sh = max(2, 14 - bd) + 1
        avg = np.clip((t0.astype(np.int32) + t1 + (1 << (sh - 1)) + 2 * 8192) >> sh, 0, (1 << bd) - 1)
        moved += int(np.count_nonzero(avg != c))
    assert moved > 1000
    # 12-bit pictures (me_util.to_bit_depth: flat areas at 0 and 4095), own generator
    bd, moved = 12, 0
    q0, q1 = (np.ascontiguousarray(np.pad(me_util.to_bit_depth(f, bd), M, mode="edge")) for f in (fr[0], fr[2]))
    rng = np.random.default_rng(1013)
    for k in range(60):
        w, h = int(rng.choice([8, 16, 32, 64, 128])), int(rng.choice([8, 16, 32, 64, 128]))
        if w * h < 128:
            continue
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        mv = [int(v) for v in rng.integers(-500, 500, 4)]
        if k % 6 == 0:
            mv[k % 4] &= ~15
        a, b, c = (np.zeros((h, w), np.int16) for _ in range(3))
        reflib.ref_bdof_pu(0, at(q0, 0, 0), at(q1, 0, 0), S, W, H, x, y, w, h, *mv, bd, ol.P(a), w)
        reflib.ref_bdof_pu(1, at(q0, 0, 0), at(q1, 0, 0), S, W, H, x, y, w, h, *mv, bd, ol.P(b), w)
        oracle.vo_bdof_pu(at(q0, x, y), S, at(q1, x, y), S, w, h, *mv, bd, ol.P(c), w)
        assert np.array_equal(a, b) and np.array_equal(a, c), (k, x, y, w, h, mv, bd)
        t0, t1 = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
        oracle.vo_mc_block(0, at(q0, x, y), S, w, h, mv[0], mv[1], 1, bd, 0, ol.P(t0), w)
        oracle.vo_mc_block(0, at(q1, x, y), S, w, h, mv[2], mv[3], 1, bd, 0, ol.P(t1), w)
        avg = np.clip((t0.astype(np.int32) + t1 + 4 + 2 * 8192) >> 3, 0, (1 << bd) - 1)
        moved += int(np.count_nonzero(avg != c))
    assert moved > 1000


def test_dmvr_equals_reference(oracle, reflib, bd=10):
    """vo_dmvr_pu vs the reference's InterPrediction::xProcessDMVR (luma; 4:0:0 rig PU): prediction and pu.mvdL0SubPu, with and without BDOF, vectors
    near the clip's motion (the refinement moves), integer / fractional phases, and far out-of-picture vectors (every clipMv call takes effect).
    8-, 10- and 12-bit pictures: the bilinear search copy and its first-pass shift depend on the depth (InterpolationFilter::filterCopy with
    biMCForDMVR, xPrefetch's bilinear filter)."""
    from vtm_amd import synth
    W, H, M = 256, 128, 160
    fr = list(synth.gen_frames(W, H, 3, seed=5))
    p0, p1 = (np.ascontiguousarray(np.pad(me_util.to_bit_depth(f, bd), M, mode="edge")) for f in (fr[0], fr[2]))
    S = p0.shape[1]
    o0, o1 = (C.c_void_p(p.ctypes.data + 2 * (M * S + M)) for p in (p0, p1))
    rng = np.random.default_rng(1014 if bd == 10 else 1014 + bd)
    moved = 0
    for k in range(160 if bd == 10 else 80):
        w, h = int(rng.choice([8, 16, 32, 64, 128])), int(rng.choice([8, 16, 32, 64, 128]))
        if w * h < 128:
            continue
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        base = np.array([48, 32]) + rng.integers(-40, 41, 2)
        mv = [int(-base[0]), int(-base[1]), int(base[0] + rng.integers(-24, 25)), int(base[1] + rng.integers(-24, 25))]
        if k % 9 == 0:
            mv = [int(v) for v in rng.integers(-4000, 4000, 4)]
        if k % 7 == 0:
            mv[0] &= ~15
        if k % 11 == 0:
            mv = [v & ~15 for v in mv]
        bio = k % 2
        nsub = (w // min(w, 16)) * (h // min(h, 16))
        a, c = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
        ma, mc = np.zeros(2 * nsub, np.int32), np.zeros(2 * nsub, np.int32)
        reflib.ref_dmvr_pu(o0, o1, S, W, H, 128, x, y, w, h, *mv, bd, bio, ol.P(a), w, C.c_void_p(ma.ctypes.data))
        oracle.vo_dmvr_pu(o0, o1, S, W, H, 128, x, y, w, h, *mv, bd, bio, ol.P(c), w, C.c_void_p(mc.ctypes.data))
        assert np.array_equal(ma, mc), (k, x, y, w, h, mv, bio)
        assert np.array_equal(a, c), (k, x, y, w, h, mv, bio)
        moved += int(np.count_nonzero(ma))
    assert moved > (500 if bd == 10 else 200), moved


def test_dmvr_420_equals_reference(oracle, reflib, bd=10):
    """Luma and both chroma planes of 4:2:0 PUs: vo_dmvr_pu + vo_dmvr_chroma vs the reference's xProcessDMVR (moved sub-PUs out of the padded chroma
    window, unmoved ones straight from the pictures); 8-, 10- and 12-bit."""
    from vtm_amd import synth
    W, H, M = 256, 128, 160
    fr = list(synth.gen_frames(W, H, 3, seed=5, chroma=True))
    P = [[np.ascontiguousarray(np.pad(me_util.to_bit_depth(f[c], bd), M if c == 0 else M // 2, mode="edge")) for c in range(3)] for f in (fr[0], fr[2])]
    SY, SC = P[0][0].shape[1], P[0][1].shape[1]
    planes = ((C.c_void_p * 3) * 2)()
    for l in range(2):
        for c in range(3):
            m, st = (M, SY) if c == 0 else (M // 2, SC)
            planes[l][c] = P[l][c].ctypes.data + 2 * (m * st + m)
    rng = np.random.default_rng(1016 if bd == 10 else 1016 + bd)
    moved = still = 0
    for k in range(120 if bd == 10 else 80):
        w, h = int(rng.choice([8, 16, 32, 64, 128])), int(rng.choice([8, 16, 32, 64, 128]))
        if w * h < 128:
            continue
        x, y = int(rng.integers(0, (W - w) // 8 + 1)) * 8, int(rng.integers(0, (H - h) // 8 + 1)) * 8
        base = np.array([48, 32]) + rng.integers(-40, 41, 2)
        mv = [int(-base[0]), int(-base[1]), int(base[0] + rng.integers(-24, 25)), int(base[1] + rng.integers(-24, 25))]
        if k % 9 == 0:
            mv = [int(v) for v in rng.integers(-4000, 4000, 4)]
        if k % 7 == 0:
            mv[0] &= ~15
        bio = k % 2
        nsub = (w // min(w, 16)) * (h // min(h, 16))
        d = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
        dp = (C.c_void_p * 3)(*[a.ctypes.data for a in d])
        ma, mc = np.zeros(2 * nsub, np.int32), np.zeros(2 * nsub, np.int32)
        reflib.ref_dmvr_pu420(planes, SY, SC, W, H, 128, x, y, w, h, *mv, bd, bio, dp, w, w // 2, C.c_void_p(ma.ctypes.data))
        c = np.zeros((h, w), np.int16)
        oracle.vo_dmvr_pu(C.c_void_p(planes[0][0]), C.c_void_p(planes[1][0]), SY, W, H, 128, x, y, w, h, *mv, bd, bio, ol.P(c), w, C.c_void_p(mc.ctypes.data))
        assert np.array_equal(ma, mc) and np.array_equal(c, d[0]), (k, x, y, w, h, mv, bio)
        for comp in (1, 2):
            e = np.zeros((h // 2, w // 2), np.int16)
            oracle.vo_dmvr_chroma(C.c_void_p(planes[0][comp]), C.c_void_p(planes[1][comp]), SC, W, H, 128, x, y, w, h, *mv, C.c_void_p(mc.ctypes.data), bd,
                                  ol.P(e), w // 2)
            assert np.array_equal(e, d[comp]), (k, comp, x, y, w, h, mv)
        mm = ma.reshape(-1, 2).any(axis=1)
        moved += int(mm.sum())
        still += int((~mm).sum())
    assert moved > (100 if bd == 10 else 40) and still > (100 if bd == 10 else 40), (moved, still)


def test_bcw_ops_equal_reference(oracle, reflib):
    """BCW variants of the two buffer ops: vo_remove_weight_high_freq vs AreaBuf::removeWeightHighFreq (scalar and x86 g_pelBufOP entries, all five
    weights incl. the negative one) and vo_add_weighted_avg vs AreaBuf::addWeightedAvg (8- and 10-bit)."""
    rng = np.random.default_rng(1018)
    weights = [reflib.ref_bcw_weight(i) for i in range(5)]
    assert weights == [-2, 3, 4, 5, 10]
    def aligned(h, stride):   # the x86 entry stores with _mm_store_si128: 16-byte aligned rows, as the encoder's buffers are
        raw = np.zeros(h * stride + 8, np.int16)
        off = (-raw.ctypes.data // 2) % 8
        return raw[off:off + h * stride].reshape(h, stride)
    for k in range(150):
        # power-of-two widths: the x86 4-wide entry touches only the first four columns of a row (x86/BufferX86.h:822-846), as removeHighFreq4 does
        w, h = int(rng.choice([4, 8, 16, 32, 64, 128])), int(rng.choice([4, 8, 16, 32, 64, 128]))
        idx = k % 5
        bw = weights[idx]
        for lw in (bw, 8 - bw):   # weight of list 1 / of list 0: both occur as the searched list
            st = max(8, w) + 8
            vals = ol.i16(rng.integers(0, 1024, (h, st)))
            pred = ol.i16(rng.integers(0, 1024, (h, w + 1)))
            a, b, c = aligned(h, st), aligned(h, st), aligned(h, st)
            a[:], b[:], c[:] = vals, vals, vals
            reflib.ref_remove_weight_high_freq(0, C.c_void_p(a.ctypes.data), st, ol.P(pred), w + 1, w, h, lw)
            reflib.ref_remove_weight_high_freq(1, C.c_void_p(b.ctypes.data), st, ol.P(pred), w + 1, w, h, lw)
            oracle.vo_remove_weight_high_freq(C.c_void_p(c.ctypes.data), st, ol.P(pred), w + 1, w, h, lw)
            assert np.array_equal(a, b) and np.array_equal(a, c), (w, h, lw)
        bd = 8 if k % 7 == 0 else 10
        hi = 8192 + ((1 << bd) - 1) * (1 << (14 - bd))
        s0, s1 = ol.i16(rng.integers(-8192, hi, (h, w))), ol.i16(rng.integers(-8192, hi, (h, w)))
        d0, d1 = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
        reflib.ref_add_weighted_avg(ol.P(s0), w, ol.P(s1), w, ol.P(d0), w, w, h, bd, idx)
        oracle.vo_add_weighted_avg(ol.P(s0), w, ol.P(s1), w, ol.P(d1), w, w, h, bd, bw)
        assert np.array_equal(d0, d1), (w, h, idx, bd)
    # 12-bit addWeightedAvg, own generator: the whole 14-bit range of a 12-bit prediction, a third of the samples at its two ends
    rng, bd = np.random.default_rng(1020), 12
    hi = 8192 + ((1 << bd) - 1) * (1 << (14 - bd))
    for k in range(60):
        w, h = int(rng.choice([4, 8, 16, 32, 64, 128])), int(rng.choice([4, 8, 16, 32, 64, 128]))
        s0, s1 = ol.i16(rng.integers(-8192, hi + 1, (h, w))), ol.i16(rng.integers(-8192, hi + 1, (h, w)))
        s0[rng.random((h, w)) < 0.33], s1[rng.random((h, w)) < 0.33] = hi, -8192
        for idx in range(5):
            d0, d1 = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
            reflib.ref_add_weighted_avg(ol.P(s0), w, ol.P(s1), w, ol.P(d0), w, w, h, bd, idx)
            oracle.vo_add_weighted_avg(ol.P(s0), w, ol.P(s1), w, ol.P(d1), w, w, h, bd, weights[idx])
            assert np.array_equal(d0, d1), (w, h, idx, bd)


def test_lfnst_equals_reference(oracle, reflib):
    """vo_fwd_lfnst / vo_inv_lfnst vs the real TrQuant::fwdLfnstNxN / invLfnstNxN for every (mode, index, size, zeroOutSize)."""
    m8, m4 = np.zeros((4, 2, 16, 48), np.int8), np.zeros((4, 2, 16, 16), np.int8)
    reflib.ref_lfnst_tables(C.c_void_p(m8.ctypes.data), C.c_void_p(m4.ctypes.data))
    assert np.abs(m8).max() > 64 and np.abs(m4).max() > 64
    rng = np.random.default_rng(1021)
    for mode in range(4):
        for index in range(2):
            for size in (4, 8):
                for zo in (8, 16):
                    for inverse in (0, 1):
                        for rep in range(6):
                            n = 48 if size > 4 else 16
                            s_ = np.zeros(48, np.int32)
                            lim = 32768 if rep == 0 else 3000
                            s_[:(zo if inverse else n)] = rng.integers(-lim, lim, zo if inverse else n)
                            a, b = np.zeros(48, np.int32), np.zeros(48, np.int32)
                            reflib.ref_lfnst(inverse, ol.P(s_), ol.P(a), mode, index, size, zo)
                            M = np.ascontiguousarray(m8[mode, index] if size > 4 else m4[mode, index])
                            (oracle.vo_inv_lfnst if inverse else oracle.vo_fwd_lfnst)(ol.P(s_), ol.P(b), C.c_void_p(M.ctypes.data), size, zo)
                            assert np.array_equal(a[:n], b[:n]), (mode, index, size, zo, inverse)


MTS_TYPES = {0: (0, 0), 2: (2, 2), 3: (1, 2), 4: (2, 1), 5: (1, 1)}   # tu.mtsIdx -> (typeHor, typeVer), TrQuant::getTrTypes (TrQuant.cpp:762-771)


def test_xT_xIT_2d_composition_equals_reference_members(oracle, reflib):
    """The real TrQuant::xT / xIT (TrQuant.cpp:776-923: shift1 / shift2, skipWidth / skipHeight, transposed passes, Pel truncation) on a rig
    TU vs the oracle's vo_fwd_2d / vo_inv_2d -- pins the 2-D COMPOSITION, not only the 1-D fast* slots."""
    rng = np.random.default_rng(881)
    n = 0
    for w in (4, 8, 16, 32, 64):
        for h in (4, 8, 16, 32, 64):
            for mts in (0, 2, 3, 4, 5):
                if mts and max(w, h) > 32:
                    continue
                th, tv = MTS_TYPES[mts]
                for bd in (8, 10):
                    amp = int(rng.choice([3, 100, (1 << bd) - 1]))
                    stride = w + int(rng.integers(0, 9))
                    resi = rng.integers(-amp, amp + 1, (h, stride)).astype(np.int16)
                    c_ref, c_or = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
                    reflib.ref_xT(ol.P(resi), stride, w, h, bd, mts, ol.P(c_ref))
                    assert oracle.vo_fwd_2d(ol.P(resi), stride, w, h, bd, th, tv, ol.P(c_or)) == 0
                    assert np.array_equal(c_ref, c_or), ("xT", w, h, mts, bd)
                    # inverse of quantisation-like coefficients (sparse, 16-bit range as Quant::dequant clips them)
                    coef = (c_ref // int(rng.choice([1, 7, 40]))).astype(np.int32)
                    coef[rng.random(w * h) < 0.3] = int(rng.integers(-32768, 32768))
                    c2 = coef.reshape(h, w)
                    zw = 16 if (th != 0 and w == 32) else max(0, w - 32)
                    zh = 16 if (tv != 0 and h == 32) else max(0, h - 32)
                    if zw:
                        c2[:, w - zw:] = 0
                    if zh:
                        c2[h - zh:, :] = 0
                    r_ref, r_or = np.zeros((h, stride), np.int16), np.zeros((h, stride), np.int16)
                    reflib.ref_xIT(ol.P(coef), w, h, bd, mts, ol.P(r_ref), stride)
                    assert oracle.vo_inv_2d(ol.P(coef), w, h, bd, th, tv, ol.P(r_or), stride) == 0
                    assert np.array_equal(r_ref[:, :w], r_or[:, :w]), ("xIT", w, h, mts, bd)
                    n += 1
    assert n == 178


def test_xT_xIT_2d_composition_12bit_extremes_equal_reference_members(oracle, reflib):
    """The 2-D composition at 12 bits: random residuals of every amplitude class, and residuals of +-4095 whose signs follow a DCT-2 / DST-7 / DCT-8 basis
    row (DCT-2 row 0 is the full-scale DC block: 4095 * 8 = 32760 after the first 4-point pass).  The inverse gets coefficients at the int16 limits."""
    rng = np.random.default_rng(884)
    bd, amp_max, n = 12, 4095, 0
    for w in (4, 8, 16, 32, 64):
        for h in (4, 8, 16, 32, 64):
            for mts in (0, 2, 3, 4, 5):
                if mts and max(w, h) > 32:
                    continue
                th, tv = MTS_TYPES[mts]
                blocks = [rng.integers(-a, a + 1, (h, w)).astype(np.int16) for a in (3, 100, amp_max)]
                for rh, rv in ((0, 0), (int(rng.integers(0, min(w, 32))), int(rng.integers(0, min(h, 32)))), (1, 0)):
                    blocks.append(ol.basis_sign_block(w, h, th, tv, rh, rv, amp_max))
                blocks.append(-blocks[-3])
                for resi in blocks:
                    c_ref, c_or = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
                    reflib.ref_xT(ol.P(resi), w, w, h, bd, mts, ol.P(c_ref))
                    assert oracle.vo_fwd_2d(ol.P(resi), w, w, h, bd, th, tv, ol.P(c_or)) == 0
                    assert np.array_equal(c_ref, c_or), ("xT", w, h, mts)
                    coef = np.clip(c_ref // int(rng.choice([1, 7])), -32768, 32767).astype(np.int32)
                    coef[rng.random(w * h) < 0.3] = rng.choice([-32768, 32767], 1)[0]
                    c2 = coef.reshape(h, w)
                    zw = 16 if (th != 0 and w == 32) else max(0, w - 32)
                    zh = 16 if (tv != 0 and h == 32) else max(0, h - 32)
                    if zw:
                        c2[:, w - zw:] = 0
                    if zh:
                        c2[h - zh:, :] = 0
                    r_ref, r_or = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
                    reflib.ref_xIT(ol.P(coef), w, h, bd, mts, ol.P(r_ref), w)
                    assert oracle.vo_inv_2d(ol.P(coef), w, h, bd, th, tv, ol.P(r_or), w) == 0
                    assert np.array_equal(r_ref, r_or), ("xIT", w, h, mts)
                    n += 1
    assert n == 89 * 7


def test_mts_preselection_equals_reference_transformNxN(oracle, reflib, bd=10):
    """The real TrQuant::transformNxN( tu, compID, cQP, &trModes, maxCand ) (TrQuant.cpp:950-1019) incl. the transform-skip candidate
    (xTransformSkip + scaleSAD) vs vtmhip_mts_select2 (host-only entry of libvtmhip.so) fed with the oracle's sum |coef| / sum |residual|."""
    from vtm_amd import lib
    L = lib.load()
    rng = np.random.default_rng(882 if bd == 10 else 882 + bd)
    n_pruned = 0
    for it in range(400 if bd == 10 else 200):
        w, h = int(rng.choice([4, 8, 16, 32])), int(rng.choice([4, 8, 16, 32]))
        # trModes as EncCu / InterSearch build them: DCT2 first, then (optionally) transform skip at position 1, then the four MTS pairs
        modes = [0] + ([1] if rng.random() < 0.6 else []) + [2, 3, 4, 5][:int(rng.integers(0, 5))]
        max_cand = int(rng.integers(0, 5))
        kind = it % 4
        amp = int(rng.choice([2, 20, 300])) << max(0, bd - 10) >> max(0, 10 - bd)
        resi = rng.integers(-amp, amp + 1, (h, w)).astype(np.int16)
        if kind == 1:     # smooth ramp: DCT2 wins by a margin, the others get pruned
            resi = (np.add.outer(np.arange(h), np.arange(w)) * amp // 8).astype(np.int16)
        elif kind == 2:   # a few isolated samples: transform skip territory
            resi[:] = 0
            resi[rng.integers(0, h, 3), rng.integers(0, w, 3)] = amp * 3
        sums = np.zeros(len(modes), np.int32)
        for i, m in enumerate(modes):
            if m == 1:
                sums[i] = int(np.abs(resi.astype(np.int64)).sum())
            else:
                coef = np.zeros(w * h, np.int32)
                th, tv = MTS_TYPES[m]
                assert oracle.vo_fwd_2d(ol.P(resi), w, w, h, bd, th, tv, ol.P(coef)) == 0
                sums[i] = int(np.abs(coef.astype(np.int64)).sum())
        marr = np.array(modes, np.uint8)
        t_lib, t_ref = np.zeros(len(modes), np.uint8), np.zeros(len(modes), np.uint8)
        assert L.vtmhip_mts_select2(sums.ctypes.data, marr.ctypes.data, len(modes), w, h, bd, 15, max_cand, t_lib.ctypes.data) == lib.OK
        reflib.ref_transformNxN_select(ol.P(resi), w, w, h, bd, ol.P(marr), len(modes), max_cand, ol.P(t_ref))
        assert list(t_lib) == list(t_ref), (w, h, modes, max_cand, list(sums), list(t_lib), list(t_ref))
        t_o = np.zeros(len(modes), np.uint8)
        oracle.vo_mts_select(ol.P(sums), ol.P(marr), len(modes), w, h, bd, 15, max_cand, ol.P(t_o))
        assert list(t_o) == list(t_ref), ("vo_mts_select", w, h, modes, max_cand, list(sums), list(t_o), list(t_ref))
        n_pruned += int(len(modes) - t_ref.sum())
    assert n_pruned > (100 if bd == 10 else 50)   # the rule actually prunes on this content


def test_transform_skip_quant_dequant_equal_reference(oracle, reflib):
    """Quant::quant / dequant with tu.mtsIdx == MTS_SKIP (no transform shift, no sqrt(2) table) vs the oracle's isTransformSkip path."""
    rng = np.random.default_rng(883)
    for w in (4, 8, 16, 32):
        for h in (4, 8, 16, 32):
            for qp in (22, 27, 32, 37, 51):
                for irap in (0, 1):
                    c = rng.integers(-1023, 1024, w * h).astype(np.int32)   # transform-skip "coefficients" are residual samples
                    q1, d1, q2, d2 = (np.zeros(w * h, np.int32) for _ in range(4))
                    s1, s2 = C.c_int32(), C.c_int32()
                    reflib.ref_quant_dequant2(ol.P(c), w, h, 10, qp, irap, 1, ol.P(q1), C.byref(s1), ol.P(d1))
                    bq = qp + 12
                    oracle.vo_quant(ol.P(c), w, h, 10, bq // 6, bq % 6, irap, 1, ol.P(q2), None, C.byref(s2))
                    oracle.vo_dequant(ol.P(q2), w, h, 10, bq // 6, bq % 6, 1, ol.P(d2))
                    assert np.array_equal(q1, q2) and np.array_equal(d1, d2) and s1.value == s2.value, (w, h, qp, irap)


def test_get_dist_part_chroma_weight(oracle, reflib):
    """RdCost::getDistPart (RdCost.cpp:411-455): chroma distortions are scaled by the fp64 m_distortionWeight and truncated; the host mirror
    (host/vtmhip_host.hpp RdCost::getDistPart) and a trampoline apply exactly (Distortion)( weight * distFunc() )."""
    reflib.ref_get_dist_part.restype = C.c_uint64
    reflib.ref_get_dist_part.argtypes = [C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    rng = np.random.default_rng(884)
    for _ in range(300):
        w, h = int(rng.choice([4, 8, 16, 32, 64])), int(rng.choice([4, 8, 16, 32, 64]))
        o, c = ol.i16(rng.integers(0, 1024, (h, w + 3))), ol.i16(rng.integers(0, 1024, (h, w + 1)))
        comp = int(rng.integers(0, 3))
        wt = float(rng.choice([1.0, 0.7937005259840998, 1.2599210498948732, 2.0 ** (rng.integers(-6, 7) / 3.0)]))
        for kind in (0, 1, 2):
            d = ol.o_dist(kind, o, c, w, h)
            exp = d if comp == 0 else int(np.float64(wt) * np.float64(d))
            got = reflib.ref_get_dist_part(comp, wt, kind, ol.P(o), w + 3, ol.P(c), w + 1, w, h, 10)
            assert got == exp, (w, h, comp, wt, kind)


def test_amvp_helpers_equal_reference_members(oracle, reflib):
    """InterSearch::xEstimateMvPredAMVP (template cost of the AMVP candidates, hook B7) and xCheckBestMVP as the real members vs the oracle."""
    import me_util
    scene = me_util.Scene(416, 240, hard=True)
    jobs = me_util.random_mest_jobs(scene, 300, seed=910)
    rng = np.random.default_rng(911)
    n_switch = 0
    for k, j in enumerate(jobs):
        j["bi"] = 0
        if k % 5 == 0:    # candidates far outside the picture: clipMv takes effect
            j["cands"][0] = [me_util._round_amvr(int(rng.integers(-9000, 9000)), j["imv"]), me_util._round_amvr(int(rng.integers(-9000, 9000)), j["imv"])]
            j["mvPred"] = tuple(j["cands"][j["mvpIdx"]])
        keep = []
        t = me_util.oracle_mest_job(scene, j, keep)
        a, b = [C.c_int(), C.c_int(), C.c_int(), C.c_uint64()], [C.c_int(), C.c_int(), C.c_int(), C.c_uint64()]
        oracle.vo_estimate_mvp_amvp(C.byref(t), *[C.byref(x) for x in a])
        reflib.ref_estimate_mvp_amvp(C.byref(t), *[C.byref(x) for x in b])
        assert [x.value for x in a] == [x.value for x in b], (j, [x.value for x in a], [x.value for x in b])
        # xCheckBestMVP on a vector near one of the candidates
        c = j["cands"][int(rng.integers(0, 2))]
        shift = {0: 2, 1: 4, 2: 6, 3: 3}[j["imv"]]
        mvh, mvv = ((c[0] >> shift) + int(rng.integers(-3, 4))) << shift, ((c[1] >> shift) + int(rng.integers(-3, 4))) << shift
        cands = ((C.c_int * 2) * 2)((C.c_int * 2)(*j["cands"][0]), (C.c_int * 2)(*j["cands"][1]))
        idxb = (C.c_uint * 2)(*j["idxBits"])
        out = []
        for fn in (oracle.vo_check_best_mvp, reflib.ref_check_best_mvp):
            ph, pv, idx = C.c_int(j["mvPred"][0]), C.c_int(j["mvPred"][1]), C.c_int(j["mvpIdx"])
            bits, cost = C.c_uint(j["bits"] + 40), C.c_uint64(100000 + int(j["lam"] * (j["bits"] + 40)))
            fn(C.c_double(j["lam"]), j["imv"], j["numCand"], cands, idxb, mvh, mvv, C.byref(ph), C.byref(pv), C.byref(idx), C.byref(bits), C.byref(cost))
            out.append((ph.value, pv.value, idx.value, bits.value, cost.value))
        assert out[0] == out[1], (j, out)
        n_switch += out[0][2] != j["mvpIdx"]
    assert n_switch > 20


def test_affine_prediction_and_me_equal_reference_members(oracle, reflib, bd=10):
    """InterPrediction::xPredAffineBlk (4x4 sub-block vectors, 6-tap sub-block filter, PROF), solveEqual and the whole
    InterSearch::xAffineMotionEstimation (gradient iterations + control-point refinement) as the real members vs the oracle; 8-, 10- and 12-bit pictures."""
    import me_util
    scene = me_util.Scene(416, 240, hard=False) if bd == 10 else me_util.DeepScene(416, 240, hard=False, bit_depth=bd)
    nj = 160 if bd == 10 else 60
    jobs = me_util.random_affine_jobs(scene, nj, seed=31 if bd == 10 else 31 + bd, bit_depth=bd)
    n_prof = n_iter = n_ref = 0
    for k, j in enumerate(jobs):
        p = me_util.affine_pred_struct(scene, j, bd)
        mv = ((C.c_int * 2) * 3)(*[(C.c_int * 2)(*v) for v in j["mv"]])
        for bi in (0, 1):
            a, b = np.zeros((j["h"], j["w"] + 3), np.int16), np.zeros((j["h"], j["w"] + 3), np.int16)
            oracle.vo_pred_affine_blk(C.byref(p), mv, bi, ol.P(a), j["w"] + 3)
            reflib.ref_pred_affine_blk(C.byref(p), mv, bi, ol.P(b), j["w"] + 3)
            assert np.array_equal(a, b), ("xPredAffineBlk", k, j, bi)
        if j["prof"]:
            p2 = me_util.affine_pred_struct(scene, dict(j, prof=0), bd)
            c = np.zeros((j["h"], j["w"] + 3), np.int16)
            oracle.vo_pred_affine_blk(C.byref(p2), mv, 0, ol.P(c), j["w"] + 3)
            n_prof += not np.array_equal(c, a if False else c) or 0
            oracle.vo_pred_affine_blk(C.byref(p), mv, 0, ol.P(a), j["w"] + 3)
            n_prof += int(not np.array_equal(a, c))
        # the whole estimation; m_hevcCost relative to the start cost decides whether the refinement stage runs
        keep = []
        t = me_util.affine_me_struct(scene, j, keep, bd)
        t.hevcCost = 1 << 62
        r0 = ol.AffineMeResult()
        oracle.vo_affine_motion_estimation(C.byref(t), C.byref(r0))
        t.hevcCost = int(r0.cost * j["hevc_scale"])
        ro, rr = ol.AffineMeResult(), ol.AffineMeResult()
        oracle.vo_affine_motion_estimation(C.byref(t), C.byref(ro))
        reflib.ref_affine_motion_estimation(C.byref(t), C.byref(rr))
        key = lambda r: ([tuple(v) for v in r.mv][:3 if j["six"] else 2], r.bits, r.cost)   # noqa: E731
        assert key(ro) == key(rr), ("xAffineMotionEstimation", k, j, key(ro), key(rr))
        n_iter += ro.iterations
        n_ref += ro.refinements
    f = 1 if bd == 10 else nj / 160
    assert n_prof > 20 * f and n_iter > 150 * f and n_ref > 500 * f, (n_prof, n_iter, n_ref)
    if bd != 10:
        return
    rng = np.random.default_rng(9)
    for _ in range(200):
        order = int(rng.choice([4, 6]))
        m = rng.integers(-10**9, 10**9, (7, 7)).astype(np.float64)
        if rng.random() < 0.2:
            m[int(rng.integers(1, order + 1))] = 0
        a, b = m.copy(), m.copy()
        pa, pb = np.zeros(6), np.zeros(6)
        oracle.vo_solve_equal(ol.P(a), order, ol.P(pa))
        reflib.ref_solve_equal(ol.P(b), order, ol.P(pb))
        assert np.array_equal(pa, pb)


def test_lfnst_scan_positions_equal_reference_tables(oracle, reflib):
    """the coefficient-scan positions of the LFNST gather / scatter: oracle (loop) and libvtmhip.so (table) vs g_coefTopLeftDiagScan8x8 / g_scanOrder"""
    from vtm_amd import lib
    L = lib.load()
    for w in (4, 8, 16, 32, 64):
        for h in (4, 8, 16, 32, 64):
            n = 48 if (w >= 8 and h >= 8) else 16
            a, b, c = np.zeros(48, np.int32), np.zeros(48, np.int32), np.zeros(48, np.int32)
            reflib.ref_lfnst_scan(w, h, ol.P(a))
            oracle.vo_lfnst_scan(w, h, ol.P(b))
            assert L.vtmhip_lfnst_scan_host(w, h, c.ctypes.data) == lib.OK
            assert np.array_equal(a[:n], b[:n]) and np.array_equal(a[:n], c[:n]), (w, h, a[:n], b[:n], c[:n])


def test_smvd_members_equal_reference(oracle, reflib):
    """InterSearch::xGetSymmetricCost, xSymmetricMotionEstimation (diamond + cross rounds of xSymmeticRefineMvSearch) and symmvdCheckBestMvp as the real
    members (two reference pictures aliasing the caller's planes) vs the oracle: all AMVR modes, SAD / SATD, clipped target, BCW weights."""
    import me_util
    for hard, bd in ((False, 10), (True, 10), (True, 8), (True, 12)):
        scene = me_util.SmvdScene(416, 240, hard=hard, bit_depth=bd)
        jobs = me_util.random_smvd_jobs(scene, 200 if bd == 10 else 80, seed=9 + hard + bd)
        moved = switched = 0
        for k, j in enumerate(jobs):
            a, b = me_util.smvd_member_results(scene, j, oracle, "vo_"), me_util.smvd_member_results(scene, j, reflib, "ref_")
            assert a == b, (k, j, a, b)
            moved += a[1][0] != tuple(j["starts"][0])
            switched += a[2][2] != (0, 0)
        assert moved > (60 if bd == 10 else 20) and switched > (15 if bd == 10 else 4), (moved, switched)


@pytest.mark.parametrize("bd", [8, 12])
def test_pred_inter_blk_luma_and_chroma_8_12bit(oracle, reflib, bd):
    """test_pred_inter_blk_luma_and_chroma at 8 and 12 bits."""
    test_pred_inter_blk_luma_and_chroma(oracle, reflib, bd)


@pytest.mark.parametrize("bd", [8, 12])
def test_dmvr_equals_reference_8_12bit(oracle, reflib, bd):
    """test_dmvr_equals_reference at 8 and 12 bits."""
    test_dmvr_equals_reference(oracle, reflib, bd)


@pytest.mark.parametrize("bd", [8, 12])
def test_dmvr_420_equals_reference_8_12bit(oracle, reflib, bd):
    """test_dmvr_420_equals_reference at 8 and 12 bits."""
    test_dmvr_420_equals_reference(oracle, reflib, bd)


@pytest.mark.parametrize("bd", [8, 12])
def test_mts_preselection_equals_reference_transformNxN_8_12bit(oracle, reflib, bd):
    """test_mts_preselection_equals_reference_transformNxN at 8 and 12 bits."""
    test_mts_preselection_equals_reference_transformNxN(oracle, reflib, bd)


@pytest.mark.parametrize("bd", [8, 12])
def test_affine_prediction_and_me_equal_reference_members_8_12bit(oracle, reflib, bd):
    """test_affine_prediction_and_me_equal_reference_members at 8 and 12 bits."""
    test_affine_prediction_and_me_equal_reference_members(oracle, reflib, bd)


# ---- the motion-search members at 8 / 12 bits, the reference's lambdas up to QP 63, lambdas beyond the device's 32-bit keys, and a saturated scene ---------------------------
def _tz_ref_equals_oracle(reflib, scene, jobs):
    exp = []
    for j in jobs:
        org = np.ascontiguousarray(scene.cur[j["y"]:j["y"] + j["h"], j["x"]:j["x"] + j["w"]])
        c, t, r = me_util.oracle_ctx(scene, j, org), me_util.oracle_tz_job(j), ol.MeResult()
        reflib.ref_tz_search(C.byref(c), C.byref(t), C.byref(r))
        exp.append((r.mvX, r.mvY, r.cost, r.dist))
    got = [g[:4] for g in me_util.run_oracle_tz(scene, jobs)]
    bad = [k for k in range(len(jobs)) if got[k] != exp[k]]
    assert not bad, (len(bad), [(jobs[k], got[k], exp[k]) for k in bad[:3]])
    return exp


@pytest.mark.parametrize("signed", [0, 1])
@pytest.mark.parametrize("bd", [8, 12])
def test_tz_search_equals_reference_xTZSearch_8_12bit(oracle, reflib, bd, signed):
    """xTZSearch on 8- and 12-bit pictures, plain and 2*org - pred targets, motion lambdas of QP 22 .. 63 at the depth and 6e5 / 2e7 / 3e9."""
    scene = me_util.DeepScene(416, 240, hard=True, bit_depth=bd)
    if signed:
        me_util.make_signed(scene, 40 + bd)
    jobs = me_util.random_tz_jobs(scene, 300, seed=211 + bd + signed, lams=me_util.real_lambdas(bd) + me_util.EDGE)
    for j in jobs:
        j["signed"] = signed
    cls = me_util.key_classes(jobs, bd)
    assert min(cls.values()) >= 20, cls
    _tz_ref_equals_oracle(reflib, scene, jobs)


@pytest.mark.parametrize("signed", [0, 1])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_tz_search_equals_reference_xTZSearch_saturated_scene(oracle, reflib, bd, signed):
    """Block SADs of about w * h * (2^bd - 1); over a third of the jobs 128x128 / 128x64 / 64x128 / 64x64.  At 12 bits the expected costs reach the limit of the device's
    one-word key (unsigned) and leave it (signed)."""
    scene = me_util.SaturatedScene(416, 240, bd, seed=60 + bd, signed=bool(signed))
    jobs = (me_util.random_tz_jobs(scene, 200, seed=221 + bd + signed, lams=me_util.real_lambdas(bd) + me_util.EDGE) +
            me_util.random_tz_jobs(scene, 150, seed=231 + bd + signed, sizes=me_util.BIG, lams=me_util.real_lambdas(bd)))
    for j in jobs:
        j["signed"] = signed
    assert sum(1 for j in jobs if j["w"] * j["h"] >= 128 * 64) * 3 >= len(jobs)
    cls = me_util.key_classes(jobs, bd)
    assert min(cls.values()) >= 20, cls
    exp = _tz_ref_equals_oracle(reflib, scene, jobs)
    if bd == 12:
        assert me_util.near_key_limit(jobs, [e[2] for e in exp], [e[3] for e in exp], bd, signed) >= 10


@pytest.mark.parametrize("saturated", [0, 1])
@pytest.mark.parametrize("bd", [8, 12])
def test_frac_and_full_search_equal_reference_8_12bit(oracle, reflib, bd, saturated):
    """xPatternSearchFracDIF and xPatternSearch at 8 / 12 bits: SAD and Hadamard, plain and signed (2*org - pred over the depth's whole range) targets, a natural and a
    saturated scene, lambdas of QP 22 .. 63."""
    scene = me_util.SaturatedScene(416, 240, bd, seed=70 + bd) if saturated else me_util.DeepScene(416, 240, hard=True, bit_depth=bd)
    rng = np.random.default_rng(240 + bd + saturated)
    lams = me_util.real_lambdas(bd)
    seen = set()
    for trial in range(200):
        w = int(rng.choice([8, 16, 32, 64, 128, 4, 16, 8, 32, 64]))
        h = int(rng.choice([8, 16, 32, 64, 128, 8, 4, 16]))
        if w == 4 and h == 4:
            continue
        x = int(rng.integers(0, (416 - w) // 4 + 1)) * 4
        y = int(rng.integers(0, (240 - h) // 4 + 1)) * 4
        org = np.ascontiguousarray(scene.cur[y:y + h, x:x + w])
        signed = trial % 3 == 0
        if signed:   # bi-pred ME target: other prediction over the whole range (natural scene) or dark (saturated: the full positive excursion)
            org = (2 * org.astype(np.int32) - rng.integers(0, 8 if saturated else 1 << bd, org.shape)).astype(np.int16)
        j = dict(w=w, h=h, x=x, y=y, subShift=0, lam=float(lams[trial % 5]), predHor=int(rng.integers(-64, 64)), predVer=int(rng.integers(-64, 64)))
        c = me_util.oracle_ctx(scene, j, org)
        assert c.bitDepth == bd
        ix, iy, had = int(rng.integers(-12, 12)), int(rng.integers(-12, 12)), int(trial % 4 != 0)
        seen.add((signed, had))
        a, b = ol.FracResult(), ol.FracResult()
        oracle.vo_frac_search(C.byref(c), ix, iy, had, 0, C.byref(a))
        reflib.ref_frac_search(C.byref(c), ix, iy, had, 0, C.byref(b))
        assert (a.halfX, a.halfY, a.qterX, a.qterY, a.cost) == (b.halfX, b.halfY, b.qterX, b.qterY, b.cost), (trial, w, h, signed, had)
        sr, out = ol.Range(), (C.c_int * 4)()
        oracle.vo_set_search_range(C.byref(c), ix * 16, iy * 16, 4, C.byref(sr))
        reflib.ref_set_search_range(C.byref(c), ix * 16, iy * 16, 4, out)
        assert list(out) == [sr.left, sr.right, sr.top, sr.bottom]
        c.subShift = 1 if (h > 8 and w <= 64) else 0
        m, r = ol.MeResult(), ol.MeResult()
        oracle.vo_full_search(C.byref(c), C.byref(sr), C.byref(m))
        reflib.ref_full_search(C.byref(c), out, C.byref(r))
        assert (m.mvX, m.mvY, m.cost, m.dist) == (r.mvX, r.mvY, r.cost, r.dist), (trial, w, h, signed)
    assert len(seen) == 4


@pytest.mark.parametrize("bd", [8, 12])
@pytest.mark.parametrize("use_had,fen,ext,first_stop", [(1, 1, 0, 1), (0, 1, 0, 0), (1, 0, 1, 1)])
def test_motion_estimation_equals_reference_xMotionEstimation_8_12bit(oracle, reflib, use_had, fen, ext, first_stop, bd):
    """Whole xMotionEstimation at 8 / 12 bits under the lambdas of QP 22 .. 63; the bi rows under the default pair and the BCW weights -2 / 3 / 5 / 10 in turn."""
    scene = me_util.DeepScene(416, 240, hard=True, bit_depth=bd)
    cfg = ol.MestCfg(4, use_had, fen, ext, first_stop)
    jobs = me_util.random_mest_jobs(scene, 200, seed=310 + use_had * 4 + fen * 2 + ext + bd, lams=me_util.real_lambdas(bd), bcws=(0, -2, 3, 5, 10))
    seen, weights = set(), set()
    for j in jobs:
        keep = []
        t = me_util.oracle_mest_job(scene, j, keep)
        assert t.bitDepth == bd
        a, b = ol.MestResult(), ol.MestResult()
        oracle.vo_motion_estimation(C.byref(cfg), C.byref(t), C.byref(a))
        reflib.ref_motion_estimation(C.byref(cfg), C.byref(t), C.byref(b))
        assert a.key() == b.key(), (j, a.key(), b.key())
        if not j["bi"]:
            assert (a.intX, a.intY) == (b.intX, b.intY)
        seen.add((j["bi"], j["imv"]))
        weights.add(j.get("bcw", 0))
    assert len(seen) == 8 and weights == {0, -2, 3, 5, 10}


@pytest.mark.parametrize("bd", [8, 12])
def test_smvd_members_equal_reference_8_12bit_real_lambdas(oracle, reflib, bd):
    """xGetSymmetricCost / xSymmetricMotionEstimation / symmvdCheckBestMvp at 8 / 12 bits under the lambdas of QP 22 .. 63 at the depth."""
    scene = me_util.SmvdScene(416, 240, hard=True, bit_depth=bd)
    jobs = me_util.draw_lambdas(me_util.random_smvd_jobs(scene, 120, seed=19 + bd), me_util.real_lambdas(bd), 19 + bd)
    moved = 0
    for k, j in enumerate(jobs):
        a, b = me_util.smvd_member_results(scene, j, oracle, "vo_"), me_util.smvd_member_results(scene, j, reflib, "ref_")
        assert a == b, (k, j, a, b)
        moved += a[1][0] != tuple(j["starts"][0])
    assert moved > 20, moved


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_width4_hadamard_of_a_weight_m2_target_scalar_is_the_arbiter(oracle, reflib, bd):
    """4-wide SATD of a saturated bi-pred target under the BCW weight -2 (-4 * org + 5 * pred, up to 5 * (2^bd - 1) from the reference block): the oracle equals the
    reference's scalar xGetHADs on every block.  The reference's own SIMD table entry (16-bit lanes for bitDepth <= 10) does not equal its scalar form there -- 433 / 2 181
    of 4 000 blocks at 8 / 10 bits when this was written -- which is why me_util.simd_had4_split leaves that class out of the saturated-scene xMotionEstimation pins;
    at 12 bits (32-bit SIMD path) the three agree."""
    rng = np.random.default_rng(40 + bd)
    top = (1 << bd) - 1
    split = 0
    for t in range(1500):
        w, h = 4, int(rng.choice([4, 8, 16]))
        org, pred, ref = top - rng.integers(0, 4, (h, w)), rng.integers(0, 4, (h, w)), rng.integers(0, 4, (h, w))
        m = rng.integers(0, 2, (h, w)) * (t % 2)                 # specks: dark in the original, bright in the other list's prediction
        org, pred = np.where(m, rng.integers(0, 64, (h, w)), org), np.where(m, top - rng.integers(0, 64, (h, w)), pred)
        ref = np.where(rng.integers(0, 2, (h, w)) * (t % 3 == 0), top - rng.integers(0, 64, (h, w)), ref)
        tgt, cur = ol.i16(-4 * org + 5 * pred), ol.i16(ref)
        scalar, simd, mine = ol.r_dist(1, 0, tgt, cur, w, h, bd), ol.r_dist(1, 1, tgt, cur, w, h, bd), ol.o_dist(1, tgt, cur, w, h)
        assert mine == scalar, (t, h, mine, scalar, simd)
        split += simd != scalar
    assert bd <= 10 or split == 0
    print("width-4 Hadamard, weight -2 target, %d bits: SIMD != scalar on %d of 1500 blocks" % (bd, split))


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("use_had,fen,ext,first_stop", [(1, 1, 0, 1), (0, 1, 0, 0)])
def test_motion_estimation_equals_reference_xMotionEstimation_saturated_scene(oracle, reflib, use_had, fen, ext, first_stop, bd):
    """Whole xMotionEstimation on the saturated scene: every shape + a list of 4-wide blocks, bi rows under the default pair and the BCW weights -2 / 3 / 5 / 10; only
    the class of me_util.simd_had4_split (where the reference's own two builds disagree) is left out."""
    scene = me_util.SaturatedScene(416, 240, bd, seed=60 + bd)
    cfgv = (4, use_had, fen, ext, first_stop)
    cfg = ol.MestCfg(*cfgv)
    lams = me_util.real_lambdas(bd)
    jobs = (me_util.random_mest_jobs(scene, 200, seed=330 + bd + use_had, lams=lams, bcws=(0, -2, 3, 5, 10)) +
            me_util.random_mest_jobs(scene, 100, seed=340 + bd + use_had, sizes=([4], [8, 16, 32, 64, 128]), lams=lams, bcws=(-2, 3, -2, 10)))
    left_out = [j for j in jobs if me_util.simd_had4_split(j, cfgv, bd)]
    jobs = [j for j in jobs if not me_util.simd_had4_split(j, cfgv, bd)]
    assert all(j["w"] == 4 and j["bcw"] == -2 for j in left_out) and (len(left_out) > 0) == bool(use_had and bd <= 10)
    for j in jobs:
        keep = []
        t = me_util.oracle_mest_job(scene, j, keep)
        a, b = ol.MestResult(), ol.MestResult()
        oracle.vo_motion_estimation(C.byref(cfg), C.byref(t), C.byref(a))
        reflib.ref_motion_estimation(C.byref(cfg), C.byref(t), C.byref(b))
        assert a.key() == b.key(), (j, a.key(), b.key())
    assert sum(1 for j in jobs if j["bi"] and j["w"] == 4 and j.get("bcw", 0) in (3, 10)) >= 10      # 4-wide weighted rows outside the class stay in
    assert sum(1 for j in jobs if j["bi"] and j.get("bcw", 0) == -2) >= (10 if bd == 12 or not use_had else 5)
