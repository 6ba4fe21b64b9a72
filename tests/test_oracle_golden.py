"""CPU: the plain-C oracle against the golden vectors recorded from the real reference (tests/golden/gen_golden.py).
This is what pins the oracle on machines where the reference itself is not available."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import me_util
import oracle_lib as ol

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_dist_golden(oracle):
    z = np.load(os.path.join(G, "dist.npz"))
    org, cur, st = z["org"], z["cur"], z["starts"]
    for (bi, w, h, kind, ss), e in zip(z["meta"], z["exp"]):
        o = np.ascontiguousarray(org[st[bi]:st[bi + 1]]).reshape(h, w)
        c = np.ascontiguousarray(cur[st[bi]:st[bi + 1]]).reshape(h, w)
        assert ol.o_dist(int(kind), o, c, int(w), int(h), int(ss)) == int(e), (w, h, kind, ss)


def test_mvcost_golden(oracle):
    rows = np.load(os.path.join(G, "mvcost.npz"))["rows"]
    for lam, ph, pv, cs, x, y, imv, e in rows:
        mc = ol.MvCost(lam, int(ph), int(pv), int(cs))
        assert oracle.vo_mv_cost(C.byref(mc), int(x), int(y), int(imv)) == int(e)


def test_interp_golden(oracle):
    z = np.load(os.path.join(G, "interp.npz"))
    src10, src14, out = z["src10"], z["src14"], z["out"]
    ss, off = 160, 8 * 160 + 8
    for (w, h, comp, frac, vertical, isFirst, isLast, alt, o0) in z["meta"]:
        src = src10 if isFirst else src14
        d = np.zeros((h, w), np.int16)
        if vertical:
            oracle.vo_if_ver(int(comp), C.c_void_p(src.ctypes.data + 2 * off), ss, ol.P(d), int(w), int(w), int(h), int(frac), int(isFirst),
                             int(isLast), 10, 0, 0, int(alt))
        else:
            oracle.vo_if_hor(int(comp), C.c_void_p(src.ctypes.data + 2 * off), ss, ol.P(d), int(w), int(w), int(h), int(frac), int(isLast), 10,
                             0, 0, int(alt))
        assert np.array_equal(d.reshape(-1), out[o0:o0 + w * h]), (w, h, comp, frac, vertical, isFirst, isLast, alt)


def test_transform_golden(oracle):
    z = np.load(os.path.join(G, "transform.npz"))
    for t in range(3):
        for n in (2, 4, 8, 16, 32, 64):
            m = np.zeros((n, n), np.int16)
            r = oracle.vo_tr_matrix(t, n, ol.P(m))
            key = "m_%d_%d" % (t, n)
            assert (r == 0) == (key in z.files)
            if r == 0:
                assert np.array_equal(m, z[key]), key
    src, dst = z["src"], z["dst"]
    for (t, n, line, a, b, shift, inv, o0) in z["meta"]:
        s = np.ascontiguousarray(src[o0:o0 + n * line])
        d = np.zeros(n * line, np.int32)
        if inv:
            oracle.vo_inv_trans(int(t), int(n), ol.P(s), ol.P(d), int(shift), int(line), int(a), int(b), -32768, 32767)
        else:
            oracle.vo_fwd_trans(int(t), int(n), ol.P(s), ol.P(d), int(shift), int(line), int(a), int(b))
        assert np.array_equal(d, dst[o0:o0 + n * line]), (t, n, line, a, b, shift, inv)


def test_motion_search_golden(oracle):
    z = np.load(os.path.join(G, "me.npz"))
    scene = me_util.Scene(416, 240, hard=True)
    jobs = [json.loads(s) for s in z["tz_jobs"]]
    got = me_util.run_oracle_tz(scene, jobs)
    for g, e in zip(got, z["tz_res"]):
        assert g[:4] == tuple(int(v) for v in e)
    for fj, fr, fu in zip(z["frac_jobs"], z["frac_res"], z["full_res"]):
        w, h, x, y, lam, ph, pv, ix, iy, had = fj
        j = dict(w=int(w), h=int(h), x=int(x), y=int(y), subShift=0, lam=float(lam), predHor=int(ph), predVer=int(pv))
        org = np.ascontiguousarray(scene.cur[j["y"]:j["y"] + j["h"], j["x"]:j["x"] + j["w"]])
        c = me_util.oracle_ctx(scene, j, org)
        r = ol.FracResult()
        oracle.vo_frac_search(C.byref(c), int(ix), int(iy), int(had), 0, C.byref(r))
        assert (r.halfX, r.halfY, r.qterX, r.qterY, r.cost) == tuple(int(v) for v in fr)
        sr = ol.Range()
        oracle.vo_set_search_range(C.byref(c), int(ix) * 16, int(iy) * 16, 4, C.byref(sr))
        assert (sr.left, sr.right, sr.top, sr.bottom) == tuple(int(v) for v in fu[:4])
        c.subShift = 1 if (j["h"] > 8 and j["w"] <= 64) else 0
        m = ol.MeResult()
        oracle.vo_full_search(C.byref(c), C.byref(sr), C.byref(m))
        assert (m.mvX, m.mvY, m.cost, m.dist) == tuple(int(v) for v in fu[4:])


def test_misc_golden(oracle):
    z = np.load(os.path.join(G, "misc.npz"))
    for k in range(int(z["count"][0])):
        pred, resi = z["pred_%d" % k], z["resi_%d" % k]
        h, w = pred.shape
        for vertical, key in ((0, "gx_%d"), (1, "gy_%d")):
            g = np.zeros((h, w), np.int32)
            oracle.vo_sobel(vertical, ol.P(pred), w, ol.P(g), w, w, h)
            assert np.array_equal(g, z[key % k])
        for six in (0, 1):
            eq = np.zeros((7, 7), np.int64)
            oracle.vo_equal_coeff(ol.P(resi), w, ol.P(z["gx_%d" % k]), ol.P(z["gy_%d" % k]), w, ol.P(eq), w, h, six)
            assert np.array_equal(eq, z["eq_%d_%d" % (k, six)])
        o = z["org_%d" % k].copy()
        oracle.vo_remove_high_freq(ol.P(o), w, ol.P(pred), w, w, h)
        assert np.array_equal(o, z["rhf_%d" % k])
        av = np.zeros((h, w), np.int16)
        oracle.vo_add_avg(ol.P(z["a14_%d" % k]), w, ol.P(z["b14_%d" % k]), w, ol.P(av), w, w, h, 10)
        assert np.array_equal(av, z["avg_%d" % k])


def test_quant_golden(oracle):
    z = np.load(os.path.join(G, "quant.npz"))
    for (w, h, qp, irap, o0, asum) in z["meta"]:
        n = int(w * h)
        c = np.ascontiguousarray(z["coef"][o0:o0 + n])
        q, d, s = np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_int32()
        bq = int(qp) + 12
        oracle.vo_quant(ol.P(c), int(w), int(h), 10, bq // 6, bq % 6, int(irap), 0, ol.P(q), None, C.byref(s))
        oracle.vo_dequant(ol.P(q), int(w), int(h), 10, bq // 6, bq % 6, 0, ol.P(d))
        assert np.array_equal(q, z["q"][o0:o0 + n]) and np.array_equal(d, z["dq"][o0:o0 + n]) and s.value == asum, (w, h, qp, irap)


def test_motion_estimation_golden(oracle):
    """xMotionEstimation results recorded from the real member function (tests/golden/gen_golden.py gen_mest)."""
    z = np.load(os.path.join(G, "mest.npz"))
    scene = me_util.Scene(416, 240, hard=True)
    for js, cfgv, exp in zip(z["jobs"], z["cfg"], z["res"]):
        j = json.loads(str(js))
        keep = []
        t = me_util.oracle_mest_job(scene, j, keep)
        cfg = ol.MestCfg(*[int(v) for v in cfgv])
        r = ol.MestResult()
        oracle.vo_motion_estimation(C.byref(cfg), C.byref(t), C.byref(r))
        assert r.key() == tuple(int(v) for v in exp), j


def _mc_planes():
    from vtm_amd import synth
    W, H, m = 416, 240, 64
    y, u, v = synth.gen_frames(W, H, 1, chroma=True)[0]
    return synth.extend_plane(y, m), synth.extend_plane(u, m // 2)


def test_mc_golden(oracle):
    """xPredInterBlk outputs recorded from the real member function (gen_golden.py gen_mc): luma and 4:2:0 chroma."""
    z = np.load(os.path.join(G, "mc.npz"))
    (yb, yo, ys), (ub, uo, us) = _mc_planes()
    pos = 0
    for comp, x, y, w, h, mvh, mvv, bi, imv in z["meta"].tolist():
        cw, ch = (w // 2, h // 2) if comp else (w, h)
        a = np.zeros((ch, cw), np.int16)
        if comp:
            refp, st = ub.ctypes.data + 2 * (uo + (y // 2) * us + x // 2), us
        else:
            refp, st = yb.ctypes.data + 2 * (yo + y * ys + x), ys
        oracle.vo_mc_block(comp, C.c_void_p(refp), st, cw, ch, mvh, mvv, bi, 10, int(imv == 3), ol.P(a), cw)
        assert np.array_equal(a.reshape(-1), z["out"][pos:pos + cw * ch]), (comp, x, y, w, h, mvh, mvv, bi, imv)
        pos += cw * ch


def test_masked_sad_golden(oracle):
    """DF_SAD_WITH_MASK values recorded from the reference's table entry (gen_golden.py gen_masked)."""
    oracle.vo_sad_mask.restype = C.c_uint64
    z = np.load(os.path.join(G, "masked.npz"))
    plane = np.ascontiguousarray(z["plane"]).reshape(-1)
    pos = 0
    for (w, h, off, ms, sx, ms2), exp in zip(z["meta"].tolist(), z["res"].tolist()):
        org, cur = np.ascontiguousarray(z["org"][pos:pos + w * h]), np.ascontiguousarray(z["cur"][pos:pos + w * h])
        pos += w * h
        got = oracle.vo_sad_mask(ol.P(org), w, ol.P(cur), w, w, h, 0, C.c_void_p(plane.ctypes.data + 2 * off), ms, sx, ms2)
        assert got == exp, (w, h, off, ms, sx, ms2)


def test_geo_blend_golden(oracle):
    """m_weightedGeoBlk blocks recorded from the reference's x86 entry (gen_golden.py gen_geo), incl. mirrored walks and 4:2:0 chroma steps."""
    z = np.load(os.path.join(G, "geo.npz"))
    planes = np.ascontiguousarray(z["planes"])
    pos = 0
    for split, comp, w, h, mi, off, sx, ws in z["meta"].tolist():
        s0, s1 = np.ascontiguousarray(z["src0"][pos:pos + w * h]), np.ascontiguousarray(z["src1"][pos:pos + w * h])
        exp = z["out"][pos:pos + w * h]
        pos += w * h
        got = np.zeros(w * h, np.int16)
        oracle.vo_weighted_geo_blk(ol.P(s0), w, ol.P(s1), w, ol.P(got), w, w, h, C.c_void_p(planes[mi].ctypes.data + 2 * off), sx, ws, 10, 0, 1023)
        assert np.array_equal(got, exp), (split, comp, w, h)


def test_bdof_golden(oracle):
    """BDOF predictions recorded from the reference (gen_golden.py gen_bdof: xPredInterBlk(bioApplied) + applyBiOptFlow, x86 buffer ops)."""
    z = np.load(os.path.join(G, "bdof.npz"))
    planes = np.ascontiguousarray(z["planes"])
    W, H, M = z["dims"].tolist()
    S = planes.shape[2]
    pos = 0
    for x, y, w, h, a, b, c, d in z["meta"].tolist():
        got = np.zeros((h, w), np.int16)
        o = [C.c_void_p(planes[l].ctypes.data + 2 * ((M + y) * S + M + x)) for l in range(2)]
        oracle.vo_bdof_pu(o[0], S, o[1], S, w, h, a, b, c, d, 10, ol.P(got), w)
        assert np.array_equal(got.reshape(-1), z["out"][pos:pos + w * h]), (x, y, w, h, a, b, c, d)
        pos += w * h


def test_dmvr_golden(oracle):
    """DMVR predictions and sub-PU vector differences recorded from the reference's xProcessDMVR (gen_golden.py gen_dmvr; planes of bdof.npz)."""
    z, zb = np.load(os.path.join(G, "dmvr.npz")), np.load(os.path.join(G, "bdof.npz"))
    planes = np.ascontiguousarray(zb["planes"])
    W, H, M = z["dims"].tolist()
    assert zb["dims"].tolist() == [W, H, M]
    S = planes.shape[2]
    o = [C.c_void_p(planes[l].ctypes.data + 2 * (M * S + M)) for l in range(2)]
    planesC = np.ascontiguousarray(z["planesC"])
    SC = planesC.shape[3]
    pos = mpos = cpos = 0
    for x, y, w, h, a, b, c, d, bio in z["meta"].tolist():
        nsub = (w // min(w, 16)) * (h // min(h, 16))
        got, mvd = np.zeros((h, w), np.int16), np.zeros(2 * nsub, np.int32)
        oracle.vo_dmvr_pu(o[0], o[1], S, W, H, 128, x, y, w, h, a, b, c, d, 10, bio, ol.P(got), w, C.c_void_p(mvd.ctypes.data))
        assert np.array_equal(mvd, z["mvd"][mpos:mpos + 2 * nsub]), (x, y, w, h)
        assert np.array_equal(got.reshape(-1), z["out"][pos:pos + w * h]), (x, y, w, h, a, b, c, d, bio)
        for comp in range(2):   # Cb, Cr
            cgot = np.zeros((h // 2, w // 2), np.int16)
            oc = [C.c_void_p(planesC[l, comp].ctypes.data + 2 * ((M // 2) * SC + M // 2)) for l in range(2)]
            oracle.vo_dmvr_chroma(oc[0], oc[1], SC, W, H, 128, x, y, w, h, a, b, c, d, C.c_void_p(mvd.ctypes.data), 10, ol.P(cgot), w // 2)
            q = w * h // 4
            assert np.array_equal(cgot.reshape(-1), z["outc"][cpos + comp * q:cpos + (comp + 1) * q]), (comp, x, y, w, h)
        cpos += w * h // 2
        pos += w * h
        mpos += 2 * nsub


def test_lfnst_golden(oracle):
    """LFNST kernels recorded from TrQuant::fwdLfnstNxN / invLfnstNxN (gen_golden.py gen_lfnst); the core matrices travel as input data."""
    z = np.load(os.path.join(G, "lfnst.npz"))
    m8, m4 = np.ascontiguousarray(z["m8"]), np.ascontiguousarray(z["m4"])
    for (inverse, mode, index, size, zo), s_, e in zip(z["meta"].tolist(), z["src"], z["out"]):
        M = m8[mode, index] if size > 4 else m4[mode, index]
        n = 48 if size > 4 else 16
        got = np.zeros(48, np.int32)
        fn = oracle.vo_inv_lfnst if inverse else oracle.vo_fwd_lfnst
        fn(ol.P(np.ascontiguousarray(s_)), ol.P(got), C.c_void_p(np.ascontiguousarray(M).ctypes.data), size, zo)
        assert np.array_equal(got[:n], e[:n]), (inverse, mode, index, size, zo)


def test_affine_me_golden(oracle):
    """golden xPredAffineBlk / xAffineMotionEstimation results recorded from the real members (tests/golden/affine_me.npz) vs the oracle"""
    import json
    import me_util
    z = np.load(os.path.join(G, "affine_me.npz"))
    scene = me_util.Scene(416, 240, hard=False)
    jobs = [json.loads(str(s)) for s in z["jobs"]]
    off = 0
    for k, j in enumerate(jobs):
        keep = []
        t = me_util.affine_me_struct(scene, j, keep)
        t.hevcCost = int(z["hevc"][k])
        r = ol.AffineMeResult()
        oracle.vo_affine_motion_estimation(C.byref(t), C.byref(r))
        n = 3 if j["six"] else 2
        assert [list(v) for v in r.mv][:n] == z["mv"][k][:n].tolist() and r.bits == int(z["bits"][k]) and r.cost == int(z["cost"][k]), (k, j)
        p = me_util.affine_pred_struct(scene, j)
        mv = ((C.c_int * 2) * 3)(*[(C.c_int * 2)(*v) for v in j["mv"]])
        a = np.zeros((j["h"], j["w"]), np.int16)
        oracle.vo_pred_affine_blk(C.byref(p), mv, 0, ol.P(a), j["w"])
        assert np.array_equal(a.reshape(-1), z["pred"][off:off + j["w"] * j["h"]]), (k,)
        off += j["w"] * j["h"]


def smvd_flat(res):
    c0, me, chk = res
    return [c0, *me[0], *me[1], me[2], *chk[0], *chk[1], *chk[2], chk[3]]


def test_smvd_golden(oracle):
    """golden xGetSymmetricCost / xSymmetricMotionEstimation / symmvdCheckBestMvp results recorded from the real members (tests/golden/smvd.npz) vs the oracle"""
    import json
    import me_util
    z = np.load(os.path.join(G, "smvd.npz"))
    scene = me_util.SmvdScene(416, 240)
    for k, s in enumerate(z["jobs"]):
        j = json.loads(str(s))
        assert smvd_flat(me_util.smvd_member_results(scene, j, oracle, "vo_")) == z["out"][k].tolist(), (k, j)


@pytest.mark.parametrize("name,min_rows,min_cached", [("pis_enc.npz", 450, 300), ("pis_enc_ldp.npz", 150, 50), ("pis_enc_ldb.npz", 150, 50)])
def test_oracle_members_on_real_encoder_records(name, min_rows, min_cached):
    """tests/golden/pis_enc*.npz (random access, low-delay P, low-delay B; predInterSearch calls recorded INSIDE the real encoder, tests/golden/gen_pis_golden.py): the oracle's xEstimateMvPredAMVP and xMotionEstimation
    on the encoder's own inputs -- real AMVP lists, m_uniMvList start vectors, block-vector cache hits (the fast-settings TZ path), the four AMVR modes, every PU shape the
    encoder tried -- against what the reference's members returned there."""
    import pis_golden as G
    L = ol.oracle()
    planes, recs = G.load_npz(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    dpb, bases = G.build_dpb(planes)
    rows = cached = 0
    for hd, sin, sout, org, fin in recs:
        cfg = ol.MestCfg(hd.bipredSearchRange, hd.useHadME, hd.fen13, hd.extendedSettings, hd.firstSearchStop)
        org = np.ascontiguousarray(org)
        for row in range(hd.numRef[0] + hd.numRef[1]):
            j, e, pl = sin.uniJobs[row], sout.uniJobs[row], planes[hd.rowPlane[row]][0]
            t = ol.MestJob()
            t.org, t.orgStride = org.ctypes.data, hd.w
            t.ref, t.refStride = dpb.ctypes.data + 2 * (bases[hd.rowPlane[row]] + hd.rowOff[row]), pl.stride
            t.w, t.h, t.puX, t.puY, t.picW, t.picH, t.ctuSize, t.bitDepth = hd.w, hd.h, j.puX, j.puY, hd.picW, hd.picH, hd.ctuSize, hd.bitDepth
            t.bi, t.imv, t.numAmvpCand, t.searchRange, t.motionLambda = 0, hd.imv, j.numAmvpCand, j.searchRange, j.motionLambda
            for i in range(2):
                t.amvpCand[i][0], t.amvpCand[i][1], t.mvpIdxBits[i] = j.amvpCand[i][0], j.amvpCand[i][1], j.mvpIdxBits[i]
            t.numExtraStart = j.numExtraStart
            for i in range(j.numExtraStart):
                t.extraStart[i][0], t.extraStart[i][1] = j.extraStart[i][0], j.extraStart[i][1]
            idx, ph, pv, dist = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
            L.vo_estimate_mvp_amvp(C.byref(t), C.byref(idx), C.byref(ph), C.byref(pv), C.byref(dist))
            assert (idx.value, ph.value, pv.value, dist.value) == (e.mvpIdx, e.mvPredHor, e.mvPredVer, sout.distBiP[row]), ("amvp", hd.poc, hd.x, hd.y, hd.w, hd.h, row)
            if not hd.rowCalls[row]:
                continue
            t.mvpIdx, t.mvPredHor, t.mvPredVer, t.bits = e.mvpIdx, e.mvPredHor, e.mvPredVer, e.bits      # the row as xMotionEstimation receives it
            t.cachedIntMv, t.mvHor, t.mvVer = int(hd.rowCached[row]), j.mvHor, j.mvVer
            r, o = ol.MestResult(), sout.uniOut[row]
            L.vo_motion_estimation(C.byref(cfg), C.byref(t), C.byref(r))
            assert (r.mvHor, r.mvVer, r.mvPredHor, r.mvPredVer, r.mvpIdx, r.bits, r.cost) == (o.mvHor, o.mvVer, o.mvPredHor, o.mvPredVer, o.mvpIdx, o.bits, o.cost), \
                ("uni", hd.poc, hd.x, hd.y, hd.w, hd.h, hd.imv, row, hd.rowCached[row])
            rows += 1
            cached += hd.rowCached[row]
    print(name, "rows", rows, "cached", cached)
    assert rows >= min_rows and cached >= min_cached, (rows, cached)


@pytest.mark.parametrize("sat", [0, 1])
@pytest.mark.parametrize("bd", [8, 12])
def test_motion_search_8_12bit_golden(oracle, bd, sat):
    """xTZSearch and xMotionEstimation at 8 / 12 bits on a natural and a saturated scene under the lambdas of QP 22 .. 63, recorded from the real members
    (tests/golden/gen_me_depth_golden.py): the oracle without the reference."""
    from test_gpu_me_depth_golden import load
    scene, jobs, exp, _ = load("tz", bd, sat)
    assert [g[:4] for g in me_util.run_oracle_tz(scene, jobs)] == exp
    scene, jobs, exp, cfgv = load("mest", bd, sat)
    got, got_int = me_util.run_oracle_mest(scene, jobs, cfgv)
    assert [g + ((0, 0) if j["bi"] else i[:2]) for g, i, j in zip(got, got_int, jobs)] == exp
