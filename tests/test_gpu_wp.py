"""GPU: explicit weighted prediction -- the weighted distortion entries (vtmhip_xGetSADw / xGetSSEw / xGetHADsw, vtmhip_wp_dist_batch_dev) and the sample
ops (vtmhip_wp_pred_batch_dev) -- against the numpy restatement in tests/wp_util.py, the reference golden tests/golden/wp.npz, the plain distortion
entries, and the C++ host mirror."""
import os
import subprocess

import numpy as np
import pytest

import wp_util as wu
from vtm_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SHAPES = {wu.SAD: wu.SAD_SHAPES, wu.SSE: wu.SSE_SHAPES, wu.SATD: wu.HAD_SHAPES}


def _pointer(ctx, kind, org, cur, wp, bd, bi, md=wu.U64):
    h, w = org.shape
    if kind == wu.SAD:
        return ctx.xGetSADw(org, w, cur, w, w, h, wp, bd, bi, md)
    return (ctx.xGetSSEw if kind == wu.SSE else ctx.xGetHADsw)(org, w, cur, w, w, h, wp, bd, bi)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_pointer_entries_match_rule(ctx, bd):
    rng = np.random.default_rng(300 + bd)
    for kind in (wu.SAD, wu.SATD, wu.SSE):
        for bi in (0, 1):
            for (w, h) in SHAPES[kind]:
                org, cur = wu.random_block(rng, w, h, bd, bi, wide=rng.random() < 0.25)
                for wp in (wu.random_wp(rng, bd), wu.derive_uni(1 << 4, int(rng.choice([0, 127, -128])), 4, bd), wu.derive_uni(-100, 9, 0, bd)):
                    cuts = wu.max_dist_cuts(wu.sad_rows(org, cur, wp, bd, bi)) if kind == wu.SAD else [wu.U64]
                    for md in cuts:
                        assert _pointer(ctx, kind, org, cur, wp, bd, bi, md) == wu.dist_w(kind, org, cur, wp, bd, bi, md), (kind, w, h, bi, wp, md)


def _mixed_batch(rng, n):
    """n jobs of mixed kind / shape / bit depth / uni-bi / maxDist in one sample pool each for org and cur, with row padding"""
    org_pool, cur_pool, jobs, exp = [], [], [], []
    no = nc = 0
    for i in range(n):
        kind = int(rng.integers(3))
        w, h = (128, 128) if i % 400 == 0 else SHAPES[kind][int(rng.integers(len(SHAPES[kind])))]
        bd, bi = int(rng.choice([8, 10, 12])), int(rng.integers(2))
        pad = int(rng.integers(0, 5))
        org, cur = wu.random_block(rng, w + pad, h, bd, bi, wide=rng.random() < 0.1)
        wp = wu.random_wp(rng, bd)
        md = wu.U64
        if kind == wu.SAD:
            cuts = wu.max_dist_cuts(wu.sad_rows(org[:, :w], cur[:, :w], wp, bd, bi))
            md = cuts[int(rng.integers(len(cuts)))]
        jobs.append(dict(orgOff=no, curOff=nc, orgStride=w + pad, curStride=w + pad, width=w, height=h, kind=kind, bitDepth=bd, isBiPred=bi, wp=wp,
                         maxDist=md))
        exp.append((kind, org[:, :w], cur[:, :w], wp, bd, bi, md))
        org_pool.append(org.reshape(-1))
        cur_pool.append(cur.reshape(-1))
        no += org.size
        nc += cur.size
    return jobs, exp, np.concatenate(org_pool), np.concatenate(cur_pool)


def _run_dist(ctx, jobs, org, cur):
    d_org, d_cur, d_jobs = ctx.to_device(org), ctx.to_device(cur), ctx.to_device(wu.pack_dist_jobs(jobs))
    d_out = ctx.alloc(8 * len(jobs))
    ctx.wp_dist_batch(d_org.ptr, d_cur.ptr, d_jobs.ptr, len(jobs), d_out.ptr)
    out = d_out.to_host(np.uint64)
    for b in (d_org, d_cur, d_jobs, d_out):
        b.free()
    return out


def test_batch_matches_pointer_entries_and_rule(ctx):
    rng = np.random.default_rng(310)
    jobs, exp, org, cur = _mixed_batch(rng, 1200)
    out = _run_dist(ctx, jobs, org, cur)
    for i, (kind, o, c, wp, bd, bi, md) in enumerate(exp):
        e = wu.dist_w(kind, o, c, wp, bd, bi, md)
        assert int(out[i]) == e, (i, jobs[i])
        if i % 20 == 0:
            assert _pointer(ctx, kind, np.ascontiguousarray(o), np.ascontiguousarray(c), wp, bd, bi, md) == e


def _grouped_batch(rng, n):
    """n jobs for the production path of vtmhip_wp_dist_batch_dev, where several consecutive jobs share a wave: mostly small blocks, with tall ones
    mixed in so that a group holds more than 64 items and job boundaries fall on both sides of a 64-item step; every kind, uni and bi, finite maxDist cuts
    (the first, a middle, the last row), and rejected jobs (no items) in the middle of groups.  Returns the jobs, the expected outputs and the pools."""
    small = {wu.SAD: [(4, 4), (8, 4), (4, 8), (8, 8), (2, 4), (6, 2)], wu.SSE: [(4, 4), (2, 2), (8, 4), (3, 5)],
             wu.SATD: [(4, 4), (8, 8), (2, 2), (6, 2), (2, 6), (8, 4)]}
    tall = {wu.SAD: [(4, 64), (2, 128), (8, 40)], wu.SSE: [(4, 70), (2, 128)], wu.SATD: [(16, 32), (2, 100), (8, 64)]}
    kinds = rng.integers(0, 3, n)
    is_tall = rng.random(n) < 0.06
    shape = [(tall if t else small)[k][int(rng.integers(len((tall if t else small)[k])))] for k, t in zip(kinds.tolist(), is_tall.tolist())]
    bds, bis, wide = rng.choice([8, 10, 12], n), rng.integers(0, 2, n), rng.random(n) < 0.1
    sizes = np.array([w * h for w, h in shape])
    offs = np.concatenate([[0], np.cumsum(sizes)])
    total = int(offs[-1])
    mx = (1 << np.repeat(bds, sizes)).astype(np.int64)
    org = (rng.random(total) * mx).astype(np.int64)                   # [0, 2^bd)
    pred = (rng.random(total) * mx).astype(np.int64)
    cur = np.where(np.repeat(bis, sizes) == 1, 2 * org - pred, pred)   # bi: the ME target 2 * org - pred
    cur = np.where(np.repeat(wide, sizes), rng.integers(-32768, 32768, total), cur)
    org, cur = org.astype(np.int16), cur.astype(np.int16)
    bad = set(range(5, n, 97))
    jobs, exp = [], []
    for i in range(n):
        kind, (w, h), bd, bi = int(kinds[i]), shape[i], int(bds[i]), int(bis[i])
        o = org[offs[i]:offs[i + 1]].reshape(h, w)
        c = cur[offs[i]:offs[i + 1]].reshape(h, w)
        wp = wu.random_wp(rng, bd)
        md, e = wu.U64, None
        if kind == wu.SAD:
            rows = wu.sad_rows(o, c, wp, bd, bi)
            cuts = wu.max_dist_cuts(rows)
            md = cuts[int(rng.integers(len(cuts)))]
            p = np.cumsum(rows)
            e = int(p[np.argmax(p > md)]) if md < p[-1] else int(p[-1])   # the first row prefix over maxDist, else the total
        elif i not in bad:
            e = wu.dist_w(kind, o, c, wp, bd, bi)
        jobs.append(dict(orgOff=offs[i], curOff=offs[i], orgStride=w, curStride=w, width=w, height=h, kind=kind, bitDepth=bd, isBiPred=bi, wp=wp,
                         maxDist=md))
        exp.append(lib.WP_INVALID_DIST if i in bad else e)
    for i in bad:
        jobs[i].update([dict(kind=3), dict(bitDepth=13), dict(wp=(1, 0, 9, 0)), dict(kind=wu.SATD, width=3, height=2)][i % 4])
    return jobs, exp, org, cur


def test_batch_with_several_jobs_per_wave(ctx):
    """vtmhip_wp_dist_batch_dev packs G = n / (32 * CUs) jobs per wave (at most 64): a batch large enough for G = 2 runs the segmented lane scan over
    several jobs, the carry through lane 63 across 64-item steps, rejected jobs inside a group and the SADw early exit beside other jobs"""
    import torch
    n = 2 * 32 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(360)
    jobs, exp, org, cur = _grouped_batch(rng, n)
    out = _run_dist(ctx, jobs, org, cur)
    for i, e in enumerate(exp):
        assert int(out[i]) == e, (i, jobs[i])
    assert sum(j["maxDist"] != wu.U64 for j in jobs) > 500 and sum(e == lib.WP_INVALID_DIST for e in exp) > 100


def test_default_weight_equals_plain_entries(ctx):
    """w = 1 << shift, offset 0, maxDist = UINT64_MAX: xGetSADw is xGetSAD; uni SSEw of in-range samples is xGetSSE"""
    rng = np.random.default_rng(320)
    for (w, h) in [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128)]:
        org, cur = wu.random_block(rng, w, h, 10, 0)
        for ld in (0, 3, 6):
            wp = wu.derive_uni(1 << ld, 0, ld, 10)
            assert ctx.xGetSADw(org, w, cur, w, w, h, wp, 10, 0) == ctx.xGetSAD(org, w, cur, w, w, h)
            assert ctx.xGetSSEw(org, w, cur, w, w, h, wp, 10, 0) == ctx.xGetSSE(org, w, cur, w, w, h)


def test_error_statuses_and_sentinel(ctx):
    o = np.full((8, 8), 100, np.int16)
    ok = wu.derive_uni(3, 1, 2, 10)
    for kind, w, h, wp, bd, bi in [(wu.SAD, 0, 4, ok, 10, 0), (wu.SAD, 4, 129, ok, 10, 0), (wu.SSE, 4, 4, ok, 7, 0), (wu.SSE, 4, 4, ok, 13, 0),
                                   (wu.SAD, 4, 4, ok, 10, 2), (wu.SAD, 4, 4, (300, 0, 2, 2), 10, 0), (wu.SSE, 4, 4, (3, 0, 9, 0), 10, 0),
                                   (wu.SATD, 4, 4, (3, 40000, 2, 0), 10, 0), (wu.SATD, 3, 2, ok, 10, 0), (wu.SATD, 2, 5, ok, 10, 1)]:
        fn = {wu.SAD: ctx.xGetSADw, wu.SSE: ctx.xGetSSEw, wu.SATD: ctx.xGetHADsw}[kind]
        with pytest.raises(lib.VtmHipError, match="status -1"):
            fn(o, 8, o, 8, w, h, wp, bd, bi)   # rejected on the host before a sample is read
    with pytest.raises(lib.VtmHipError, match="status -1"):
        ctx.wp_dist_batch(0, 0, 0, 1, 0)
    with pytest.raises(lib.VtmHipError, match="status -1"):
        ctx.wp_pred_batch(0, 0, 0, 0, 1)
    ctx.wp_dist_batch(0, 0, 0, 0, 0)   # n = 0: nothing to do
    # device-side rejections: VTMHIP_WP_INVALID_DIST, the neighbours computed
    rng = np.random.default_rng(330)
    jobs, exp, org, cur = _mixed_batch(rng, 64)
    bad = {3: dict(kind=3), 5: dict(width=0), 9: dict(height=200), 11: dict(bitDepth=14), 17: dict(isBiPred=2), 21: dict(wp=(999, 0, 1, 0)),
           23: dict(wp=(1, 0, 12, 0)), 29: dict(kind=wu.SATD, width=3, height=6)}
    for i, kv in bad.items():
        jobs[i].update(kv)
    out = _run_dist(ctx, jobs, org, cur)
    for i, (kind, o, c, wp, bd, bi, md) in enumerate(exp):
        if i in bad:
            assert int(out[i]) == lib.WP_INVALID_DIST, i
        else:
            assert int(out[i]) == wu.dist_w(kind, o, c, wp, bd, bi, md), i


def _pred_jobs_from_golden(z):
    return [dict(src0Off=z["p_src0_off"][i], src1Off=z["p_src1_off"][i], dstOff=z["p_dst_off"][i], src0Stride=z["p_w"][i], src1Stride=z["p_w"][i],
                 dstStride=z["p_w"][i], width=z["p_w"][i], height=z["p_h"][i], bitDepth=z["p_bd"][i], mode=z["p_mode"][i], w0=z["p_wp"][i][0],
                 w1=z["p_wp"][i][1], offset=z["p_wp"][i][2], shift=z["p_wp"][i][3], round=z["p_wp"][i][4]) for i in range(len(z["p_mode"]))]


def test_golden_replay(ctx):
    z = np.load(os.path.join(ROOT, "tests", "golden", "wp.npz"))
    n = len(z["d_dist"])
    jobs = [dict(orgOff=z["d_org_off"][i], curOff=z["d_cur_off"][i], orgStride=z["d_w"][i], curStride=z["d_w"][i], width=z["d_w"][i], height=z["d_h"][i],
                 kind=z["d_kind"][i], bitDepth=z["d_bd"][i], isBiPred=z["d_bi"][i], wp=z["d_wp"][i], maxDist=z["d_max"][i]) for i in range(n)]
    assert np.array_equal(_run_dist(ctx, jobs, z["org"], z["cur"]), z["d_dist"])
    for i in range(0, n, 11):   # and through the pointer entries
        w, h = int(z["d_w"][i]), int(z["d_h"][i])
        o = z["org"][z["d_org_off"][i]:][: w * h].reshape(h, w).copy()
        c = z["cur"][z["d_cur_off"][i]:][: w * h].reshape(h, w).copy()
        got = _pointer(ctx, int(z["d_kind"][i]), o, c, tuple(int(v) for v in z["d_wp"][i]), int(z["d_bd"][i]), int(z["d_bi"][i]), int(z["d_max"][i]))
        assert got == int(z["d_dist"][i]), i
    # sample ops
    pj = _pred_jobs_from_golden(z)
    d_src, d_jobs = ctx.to_device(z["src"]), ctx.to_device(wu.pack_pred_jobs(pj))
    d_dst = ctx.to_device(np.full(z["dst"].shape, -7, np.int16))
    ctx.wp_pred_batch(d_src.ptr, d_src.ptr, d_dst.ptr, d_jobs.ptr, len(pj))
    assert np.array_equal(d_dst.to_host(np.int16), z["dst"])
    # a rejected job leaves its block untouched
    pj[0].update(shift=9)
    pj[1].update(mode=2)
    d_jobs2, d_dst2 = ctx.to_device(wu.pack_pred_jobs(pj[:3])), ctx.to_device(np.full(z["dst"].shape, -7, np.int16))
    ctx.wp_pred_batch(d_src.ptr, d_src.ptr, d_dst2.ptr, d_jobs2.ptr, 3)
    got = d_dst2.to_host(np.int16)
    for i in (0, 1):
        s, m = int(z["p_dst_off"][i]), int(z["p_w"][i] * z["p_h"][i])
        assert np.all(got[s:s + m] == -7), i
    s, m = int(z["p_dst_off"][2]), int(z["p_w"][2] * z["p_h"][2])
    assert np.array_equal(got[s:s + m], z["dst"][s:s + m])
    for b in (d_src, d_jobs, d_dst, d_jobs2, d_dst2):
        b.free()


def test_mc_intermediates_then_weighted_pred(ctx):
    """a weighted-prediction PU as two launches: vtmhip_mc_batch_dev with bi = 1 (14-bit intermediates of both lists), then vtmhip_wp_pred_batch_dev"""
    rng = np.random.default_rng(340)
    bd, W, H, M = 10, 160, 96, 16
    refs = [rng.integers(0, 1 << bd, (H + 2 * M, W + 2 * M)).astype(np.int16) for _ in range(2)]
    stride = W + 2 * M
    plane = np.concatenate([r.reshape(-1) for r in refs])
    blocks, mc, off = [], [], 0
    for i in range(48):
        w, h = [(8, 8), (16, 8), (16, 16), (32, 16), (8, 4), (64, 32)][i % 6]
        x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
        for l in range(2):
            mc.append(lib.McJob(refOff=l * refs[0].size + (y + M) * stride + x + M, dstOff=off + l * w * h, refStride=stride, dstStride=w, width=w, height=h,
                                mvHor=int(rng.integers(-64, 65)), mvVer=int(rng.integers(-64, 65)), bi=1, bitDepth=bd, useAltHpelIf=0, chroma=0))
        blocks.append((off, w, h))
        off += 2 * w * h
    d_plane, d_tmp = ctx.to_device(plane), ctx.alloc(2 * off)
    arr = (lib.McJob * len(mc))(*mc)
    d_mc = ctx.to_device(np.frombuffer(arr, np.uint8).copy())
    ctx.mc_batch(d_plane.ptr, d_tmp.ptr, d_mc.ptr, len(mc), 64, 32)
    pj, exp = [], []
    for i, (o, w, h) in enumerate(blocks):
        ld = int(rng.integers(0, 8))
        w0, io0 = (1 << ld, 0) if i % 5 == 0 else (int(rng.integers(-128, 128)), int(rng.integers(-128, 128)))
        if i % 2:
            b = wu.derive_bi(w0, io0, int(rng.integers(-128, 128)), int(rng.integers(-128, 128)), ld, bd)
            pj.append(dict(src0Off=o, src1Off=o + w * h, dstOff=o // 2, src0Stride=w, src1Stride=w, dstStride=w, width=w, height=h, bitDepth=bd, mode=lib.WP_BI,
                           w0=b[0], w1=b[1], offset=b[2], shift=b[3], round=b[4]))
        else:
            u = wu.derive_uni(w0, io0, ld, bd)
            pj.append(dict(src0Off=o, src1Off=0, dstOff=o // 2, src0Stride=w, src1Stride=w, dstStride=w, width=w, height=h, bitDepth=bd, mode=lib.WP_UNI,
                           w0=u[0], w1=0, offset=u[1], shift=u[2], round=u[3]))
    d_jobs, d_dst = ctx.to_device(wu.pack_pred_jobs(pj)), ctx.alloc(off)
    ctx.wp_pred_batch(d_tmp.ptr, d_tmp.ptr, d_dst.ptr, d_jobs.ptr, len(pj))
    tmp, dst = d_tmp.to_host(np.int16), d_dst.to_host(np.int16)
    assert tmp.min() < 0 and tmp.max() > 8192   # really the 14-bit intermediates, not samples
    for (o, w, h), j in zip(blocks, pj):
        s0 = tmp[o:o + w * h].reshape(h, w)
        s1 = tmp[o + w * h:o + 2 * w * h].reshape(h, w)
        e = (wu.add_weight_bi(s0, s1, j["w0"], j["w1"], j["offset"], j["shift"], bd) if j["mode"] == lib.WP_BI else
             wu.add_weight_uni(s0, j["w0"], j["offset"], j["shift"], bd))
        assert np.array_equal(dst[o // 2:o // 2 + w * h].reshape(h, w), e), j
    for b in (d_plane, d_tmp, d_mc, d_jobs, d_dst):
        b.free()


def test_host_mirror_weighted_slots(ctx, tmp_path):
    """host/vtmhip_host.hpp: applyWeight on the SAD / HAD / SSE / SSE_WTD slots with RdCost::setDeviceWeightedPrediction( true ), wpCur per component"""
    exe = str(tmp_path / "host_wp")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-o", exe, os.path.join(ROOT, "host", "test_host_wp.cpp"), "-L" + os.path.join(ROOT, "vtm_amd"),
                           "-lvtmhip", "-Wl,-rpath," + os.path.join(ROOT, "vtm_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(350)
    body, exp = bytearray(), []
    n = 0
    for kind in (0, 1, 2, 3):
        shapes = {0: wu.SAD_SHAPES, 1: wu.HAD_SHAPES, 2: wu.SSE_SHAPES, 3: wu.SSE_SHAPES}[kind]
        for (w, h) in shapes[:8]:
            bd, bi, comp = int(rng.choice([8, 10, 12])), int(rng.integers(2)), int(rng.integers(3))
            org, cur = wu.random_block(rng, w, h, bd, bi)
            wp = wu.random_wp(rng, bd)
            k = {0: wu.SAD, 1: wu.SATD, 2: wu.SSE, 3: wu.SSE}[kind]
            md = wu.U64
            if k == wu.SAD:
                cuts = wu.max_dist_cuts(wu.sad_rows(org, cur, wp, bd, bi))
                md = cuts[int(rng.integers(len(cuts)))]
            body += np.array([kind, w, h, bd, bi, comp, *wp], np.int32).tobytes() + np.array([md], np.uint64).tobytes() + org.tobytes() + cur.tobytes()
            exp.append(wu.dist_w(k, org, cur, wp, bd, bi, md))
            n += 1
    inp = tmp_path / "in.bin"
    inp.write_bytes(np.array([n], np.int32).tobytes() + bytes(body))
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split()
    assert lines[-2:] == ["sse-subshift-check", "refused-when-off"]
    assert [int(v) for v in lines[:-2]] == exp
