"""GPU: the luma-level-weighted SSE family (DF_SSE_WTD .. DF_SSE16N_WTD) -- pointer entry, batched entry with the fused inverse reshape, table
state, error statuses, the reference golden replay and the C++ host mirror -- against the numpy restatement in tests/wtd_util.py."""
import os
import subprocess

import numpy as np
import pytest

import wtd_util as wu
from test_gpu_dist import SIZES
from vtm_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FORMATS = list(wu.CF_SCALE.values())


def _block(rng, bd, w, h, comp, sx, sy):
    mx = 1 << bd
    org = rng.integers(0, mx, (h, w)).astype(np.int16)
    cur = np.clip(org.astype(np.int64) + rng.integers(-mx // 8, mx // 8 + 1, (h, w)), 0, mx - 1).astype(np.int16)
    luma = rng.integers(0, mx, (h << sy, w << sx)).astype(np.int16) if comp else None
    return org, cur, luma


def _pointer(ctx, org, cur, comp, luma, sx, sy):
    h, w = org.shape
    return ctx.xGetSSE_WTD(org, w, cur, w, w, h, comp, luma, 0 if luma is None else luma.shape[1], sx, sy)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("signal", [wu.SDR, wu.PQ])
def test_pointer_entry_matches_rule(ctx, bd, signal):
    rng = np.random.default_rng(10 * bd + signal)
    lut, cw = (wu.pq_table(bd) if signal == wu.PQ else wu.random_table(rng, bd)), 1.37
    ctx.set_luma_level_weights(lut, bd, signal, cw)
    for i, (w, h) in enumerate(SIZES):
        org, cur, _ = _block(rng, bd, w, h, 0, 0, 0)
        assert _pointer(ctx, org, cur, 0, None, 0, 0) == wu.sse_wtd(org, cur, 0, lut, signal, cw), (w, h)
        sx, sy = FORMATS[i % 3]
        for comp in (1, 2):
            org, cur, luma = _block(rng, bd, w, h, comp, sx, sy)
            assert _pointer(ctx, org, cur, comp, luma, sx, sy) == wu.sse_wtd(org, cur, comp, lut, signal, cw, luma, sx, sy), (w, h, comp, sx, sy)


def test_unit_weights_equal_plain_sse(ctx):
    rng = np.random.default_rng(3)
    ctx.set_luma_level_weights(np.ones(1 << 10), 10, wu.PQ, 1.0)
    for (w, h) in SIZES:
        org, cur, luma = _block(rng, 10, w, h, 1, 1, 1)
        plain = ctx.xGetSSE(org, w, cur, w, w, h)
        assert _pointer(ctx, org, cur, 0, None, 0, 0) == plain
        assert _pointer(ctx, org, cur, 1, luma, 1, 1) == plain


def test_large_weights_truncate(ctx):
    rng = np.random.default_rng(4)
    bd = 12
    lut = rng.uniform(2000.0, 32767.0, 1 << bd)
    ctx.set_luma_level_weights(lut, bd, wu.SDR, 20000.0)
    for (w, h) in [(4, 4), (16, 8), (64, 64), (128, 128), (2, 8), (6, 4)]:
        org = rng.integers(0, 4096, (h, w)).astype(np.int16)
        cur = np.where(org > 2048, 0, 4095).astype(np.int16)
        luma = rng.integers(0, 4096, (h << 1, w << 1)).astype(np.int16)
        assert _pointer(ctx, org, cur, 0, None, 0, 0) == wu.sse_wtd(org, cur, 0, lut, wu.SDR, 20000.0)
        assert _pointer(ctx, org, cur, 1, luma, 1, 1) == wu.sse_wtd(org, cur, 1, lut, wu.SDR, 20000.0, luma, 1, 1)


def _mixed_batch(rng, bd, n):
    """n jobs of mixed shape over three sample pools; a few 128x128 luma, many 2x2 / 2x4 / 4x4 chroma; half of the luma jobs inverse-reshaped."""
    mx = 1 << bd
    pools = {"org": [], "cur": [], "luma": []}
    size = {"org": 0, "cur": 0, "luma": 0}

    def put(name, a):
        off = size[name]
        pools[name].append(a.reshape(-1))
        size[name] += a.size
        return off

    shapes = [(2, 2), (2, 4), (4, 4), (4, 2), (8, 8), (6, 4), (16, 16), (12, 8), (32, 32), (64, 64), (24, 16), (48, 32)]
    jobs, exp_args = [], []
    for i in range(n):
        if i % 700 == 0:
            w, h = 128, 128
        else:
            w, h = shapes[int(rng.integers(len(shapes)))]
        comp = int(rng.integers(3)) if w < 128 else 0
        sx, sy = FORMATS[int(rng.integers(3))] if comp else (0, 0)
        pad = int(rng.integers(0, 5))
        org = rng.integers(0, mx, (h, w + pad)).astype(np.int16)
        cur = rng.integers(0, mx, (h, w + pad)).astype(np.int16)
        luma = rng.integers(0, mx, (h << sy, (w << sx) + 3)).astype(np.int16)
        flags = lib.WTD_INV_RESHAPE_CUR if comp == 0 and rng.random() < 0.5 else 0
        jobs.append(dict(orgOff=put("org", org), curOff=put("cur", cur), orgLumaOff=put("luma", luma), orgStride=w + pad, curStride=w + pad,
                         orgLumaStride=luma.shape[1], width=w, height=h, compID=comp, cShiftX=sx, cShiftY=sy, flags=flags))
        exp_args.append((org[:, :w], cur[:, :w], comp, luma, sx, sy, flags))
    return jobs, exp_args, {k: np.concatenate(v) for k, v in pools.items()}


def _run_batch(ctx, jobs, pools):
    d_org, d_cur, d_luma = (ctx.to_device(pools[k]) for k in ("org", "cur", "luma"))
    d_jobs = ctx.to_device(wu.pack_jobs(jobs))
    d_out = ctx.alloc(8 * len(jobs))
    ctx.sse_wtd_batch(d_org.ptr, d_cur.ptr, d_luma.ptr, d_jobs.ptr, len(jobs), d_out.ptr)
    out = d_out.to_host(np.uint64)
    for b in (d_org, d_cur, d_luma, d_jobs, d_out):
        b.free()
    return out


@pytest.mark.parametrize("signal", [wu.SDR, wu.PQ])
def test_batch_matches_pointer_entry_and_rule(ctx, signal):
    bd = 10
    rng = np.random.default_rng(20 + signal)
    lut, cw, inv = wu.random_table(rng, bd), 0.83, wu.random_inv_lut(rng, bd)
    ctx.set_luma_level_weights(lut, bd, signal, cw, inv)
    jobs, args, pools = _mixed_batch(rng, bd, 3000)
    out = _run_batch(ctx, jobs, pools)
    for i, (org, cur, comp, luma, sx, sy, flags) in enumerate(args):
        exp = wu.sse_wtd(org, cur, comp, lut, signal, cw, luma, sx, sy, inv if flags else None)
        assert int(out[i]) == exp, (i, jobs[i])
        if i % 5 == 0:   # the pointer entry on the same blocks (cur mapped on the host for the reshape flag, as the reference's callers do)
            c = inv[cur] if flags else np.ascontiguousarray(cur)
            assert _pointer(ctx, np.ascontiguousarray(org), c.astype(np.int16), comp, luma, sx, sy) == exp


PACKED_SMALL, PACKED_TALL = [(2, 2), (2, 4), (4, 4), (6, 4), (8, 8)], [(4, 70), (12, 40), (6, 50)]   # tall: 70 / 120 / 100 row segments, no multiple of 64
PACKED_REJECT = [dict(compID=3), dict(width=0), dict(flags=4)]


def _packed_batch(rng, bd, n, lut, cw, inv):
    """n PQ jobs for groups of two: mostly small blocks of all components and chroma formats, ~6 % tall ones (i % 32 == 20: the first job of its group, == 3: the
    second), half of the luma jobs inverse-reshaped, every 97th rejected.  The expectations are wtd_util's rule, evaluated for all jobs of one shape at a time."""
    mx = 1 << bd
    keys = []
    for i in range(n):
        w, h = PACKED_TALL[(i // 32) % 3] if i % 32 in (3, 20) else PACKED_SMALL[int(rng.integers(len(PACKED_SMALL)))]
        comp = int(rng.integers(3))
        sx, sy = FORMATS[int(rng.integers(3))] if comp else (0, 0)
        keys.append((w, h, comp, sx, sy, lib.WTD_INV_RESHAPE_CUR if comp == 0 and i % 2 == (i // 2) % 2 else 0, int(rng.integers(0, 5))))
    pools, size = {"org": [], "cur": [], "luma": []}, {"org": 0, "cur": 0, "luma": 0}
    jobs, exp = [None] * n, [lib.WTD_INVALID_DIST] * n
    for key in sorted(set(keys)):
        w, h, comp, sx, sy, flags, pad = key
        idx = [i for i in range(n) if keys[i] == key]
        m, lw = len(idx), (w << sx) + 3
        org, cur = (rng.integers(0, mx, (m, h, w + pad)).astype(np.int16) for _ in range(2))
        luma = rng.integers(0, mx, (m, h << sy, lw)).astype(np.int16)
        lv = org[:, :, :w] if comp == 0 else luma[:, (np.arange(h) << sy)[:, None], (np.arange(w) << sx)[None, :]]
        c = inv[cur[:, :, :w]] if flags else cur[:, :, :w]
        dist = wu.mse_samples(comp, org[:, :, :w], c, lv, lut, wu.PQ, cw).astype(np.int64).astype(np.uint64).reshape(m, -1).sum(axis=1, dtype=np.uint64)
        for k, i in enumerate(idx):
            jobs[i] = dict(orgOff=size["org"] + k * org[0].size, curOff=size["cur"] + k * cur[0].size, orgLumaOff=size["luma"] + k * luma[0].size, orgStride=w + pad,
                           curStride=w + pad, orgLumaStride=lw, width=w, height=h, compID=comp, cShiftX=sx, cShiftY=sy, flags=flags)
            if i % 97 == 96:
                jobs[i].update(PACKED_REJECT[(i // 97) % 3])
            else:
                exp[i] = int(dist[k])
            if i % 50 == 0:   # the per-block form of the rule on the same samples
                assert int(dist[k]) == wu.sse_wtd(org[k, :, :w], cur[k, :, :w], comp, lut, wu.PQ, cw, luma[k], sx, sy, inv if flags else None)
        for name, a in (("org", org), ("cur", cur), ("luma", luma)):
            pools[name].append(a.reshape(-1))
            size[name] += a.size
    return jobs, exp, {k: np.concatenate(v) for k, v in pools.items()}


def test_batch_with_several_jobs_per_wave(ctx):
    """vtmhip_sse_wtd_batch_dev packs G = n / (32 * CUs) jobs per wave (at most 64): a batch large enough for G = 2 runs the cursor over two jobs per wave, a
    lane's accumulator flushed into the right job's sum when its segments move on, tall jobs whose end falls inside a 64-segment step as the first and as the
    second job of a group, and rejected jobs inside a group.  PQ: every chroma sample reads the co-located luma."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, bd = 2 * 32 * cus, 10
    assert n // (32 * cus) == 2
    rng = np.random.default_rng(60)
    lut, cw, inv = wu.random_table(rng, bd), 0.83, wu.random_inv_lut(rng, bd)
    ctx.set_luma_level_weights(lut, bd, wu.PQ, cw, inv)
    jobs, exp, pools = _packed_batch(rng, bd, n, lut, cw, inv)
    out = _run_batch(ctx, jobs, pools)
    bad = [i for i in range(n) if int(out[i]) != exp[i]]
    assert not bad, (len(bad), [(i, jobs[i], int(out[i]), exp[i]) for i in bad[:3]])
    tall = [sum(1 for i in range(first, n, 2) if (jobs[i]["width"], jobs[i]["height"]) in PACKED_TALL and exp[i] != lib.WTD_INVALID_DIST) for first in (0, 1)]
    assert min(tall) >= n // 40 and sum(e == lib.WTD_INVALID_DIST for e in exp) == n // 97
    luma_jobs = [j for j in jobs if j["compID"] == 0]
    assert abs(2 * sum(j["flags"] == lib.WTD_INV_RESHAPE_CUR for j in luma_jobs) - len(luma_jobs)) < len(luma_jobs) // 10
    assert {(j["compID"], j["cShiftX"], j["cShiftY"]) for j in jobs} >= {(0, 0, 0)} | {(c, sx, sy) for c in (1, 2) for (sx, sy) in FORMATS}


def test_table_reset_between_batches(ctx):
    bd = 8
    rng = np.random.default_rng(30)
    lut1, lut2 = wu.random_table(rng, bd), wu.random_table(rng, bd, 4.0, 5.0)
    jobs, args, pools = _mixed_batch(rng, bd, 400)
    for j in jobs:
        j["flags"] = 0
    d_org, d_cur, d_luma = (ctx.to_device(pools[k]) for k in ("org", "cur", "luma"))
    d_jobs = ctx.to_device(wu.pack_jobs(jobs))
    d1, d2 = ctx.alloc(8 * len(jobs)), ctx.alloc(8 * len(jobs))
    ctx.set_luma_level_weights(lut1, bd, wu.PQ, 1.0)
    ctx.sse_wtd_batch(d_org.ptr, d_cur.ptr, d_luma.ptr, d_jobs.ptr, len(jobs), d1.ptr)   # queued, not synchronised
    ctx.set_luma_level_weights(lut2, bd, wu.PQ, 1.0)
    ctx.sse_wtd_batch(d_org.ptr, d_cur.ptr, d_luma.ptr, d_jobs.ptr, len(jobs), d2.ptr)
    o1, o2 = d1.to_host(np.uint64), d2.to_host(np.uint64)
    for i, (org, cur, comp, luma, sx, sy, _) in enumerate(args):
        assert int(o1[i]) == wu.sse_wtd(org, cur, comp, lut1, wu.PQ, 1.0, luma, sx, sy)
        assert int(o2[i]) == wu.sse_wtd(org, cur, comp, lut2, wu.PQ, 1.0, luma, sx, sy)
    for b in (d_org, d_cur, d_luma, d_jobs, d1, d2):
        b.free()


def test_error_statuses():
    from vtm_amd.device import Context
    c = Context(0)   # a fresh context: no table yet
    try:
        o = np.full((4, 4), 100, np.int16)
        with pytest.raises(lib.VtmHipError, match="status -1"):
            _pointer(c, o, o, 0, None, 0, 0)
        with pytest.raises(lib.VtmHipError, match="status -1"):
            c.sse_wtd_batch(1, 1, 1, 1, 1, 1)   # no table: rejected before anything is read
        for bd in (7, 13):
            with pytest.raises(lib.VtmHipError, match="status -1"):
                c.set_luma_level_weights(np.ones(1 << 13), bd, wu.SDR, 1.0)
        with pytest.raises(lib.VtmHipError, match="status -1"):
            c.set_luma_level_weights(np.full(256, 40000.0), 8, wu.SDR, 1.0)   # 40000 * 65536 >= 2^31
        c.set_luma_level_weights(np.ones(256), 8, wu.SDR, 1.0)   # no inverse LUT
        luma = np.full((8, 8), 100, np.int16)
        for comp, sx, sy in ((3, 0, 0), (0, 1, 0), (1, 2, 0), (1, 0, -1)):
            with pytest.raises(lib.VtmHipError, match="status -1"):
                _pointer(c, o, o, comp, luma, sx, sy)
        with pytest.raises(lib.VtmHipError, match="status -1"):
            _pointer(c, o, o, 1, None, 1, 1)   # chroma without orgLuma
        neg = o.copy()
        neg[1, 2] = -1
        with pytest.raises(lib.VtmHipError, match="status -1"):
            _pointer(c, neg, o, 0, None, 0, 0)
        # device-side rejections of the batch: the reshape flag without an inverse LUT / on chroma, bad compID / cShift -> WTD_INVALID_DIST, the rest computed
        rng = np.random.default_rng(40)
        jobs, args, pools = _mixed_batch(rng, 8, 64)
        for j in jobs:
            j["flags"] = 0
        bad = {3: dict(flags=lib.WTD_INV_RESHAPE_CUR, compID=0, cShiftX=0, cShiftY=0), 7: dict(compID=3), 11: dict(compID=1, cShiftX=2),
               13: dict(compID=0, cShiftX=1), 17: dict(flags=4)}
        for i, kv in bad.items():
            jobs[i].update(kv)
        out = _run_batch(c, jobs, pools)
        for i, (org, cur, comp, luma, sx, sy, _) in enumerate(args):
            if i in bad:
                assert int(out[i]) == lib.WTD_INVALID_DIST, i
            else:
                assert int(out[i]) == wu.sse_wtd(org, cur, comp, np.ones(256), wu.SDR, 1.0, luma, sx, sy), i
        c.set_luma_level_weights(np.ones(256), 8, wu.SDR, 1.0, np.arange(256, dtype=np.int16))
        jobs[3].update(compID=1, cShiftX=1, cShiftY=1)   # the flag on chroma
        out = _run_batch(c, jobs[:4], pools)
        assert int(out[3]) == lib.WTD_INVALID_DIST
    finally:
        c.close()


def test_golden_replay(ctx):
    z = np.load(os.path.join(ROOT, "tests", "golden", "sse_wtd.npz"))
    for k in range(len(z["set_bd"])):
        ctx.set_luma_level_weights(z["lut%d" % k], int(z["set_bd"][k]), int(z["set_signal"][k]), float(z["set_chroma"][k]))
        sel = np.nonzero(z["c_set"] == k)[0]
        jobs = [dict(orgOff=z["c_org_off"][i], curOff=z["c_cur_off"][i], orgLumaOff=z["c_luma_off"][i], orgStride=z["c_w"][i], curStride=z["c_w"][i],
                     orgLumaStride=z["c_luma_stride"][i], width=z["c_w"][i], height=z["c_h"][i], compID=z["c_comp"][i], cShiftX=z["c_csx"][i],
                     cShiftY=z["c_csy"][i], flags=0) for i in sel]
        out = _run_batch(ctx, jobs, {"org": z["org"], "cur": z["cur"], "luma": z["luma"]})
        assert np.array_equal(out, z["c_dist"][sel]), k
        for i in sel[::4]:   # and through the pointer entry
            w, h, comp, sx, sy = (int(z[c][i]) for c in ("c_w", "c_h", "c_comp", "c_csx", "c_csy"))
            org = z["org"][z["c_org_off"][i]:][: w * h].reshape(h, w).copy()
            cur = z["cur"][z["c_cur_off"][i]:][: w * h].reshape(h, w).copy()
            ls = int(z["c_luma_stride"][i])
            luma = z["luma"][z["c_luma_off"][i]:][: (h << sy) * ls].reshape(-1, ls).copy() if comp else None
            assert _pointer(ctx, org, cur, comp, luma, sx, sy) == int(z["c_dist"][i])


def test_host_mirror_get_dist_part(ctx, tmp_path):
    """host/vtmhip_host.hpp: RdCost::getDistPart( ..., DF_SSE_WTD, &orgLuma ) through the installed slots, incl. the chroma m_distortionWeight scaling."""
    exe = str(tmp_path / "host_wtd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-o", exe, os.path.join(ROOT, "host", "test_host_wtd.cpp"), "-L" + os.path.join(ROOT, "vtm_amd"),
                           "-lvtmhip", "-Wl,-rpath," + os.path.join(ROOT, "vtm_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(50)
    bd, signal, cw, dw = 10, wu.PQ, 1.2, (1.0, 0.7734, 1.3311)
    lut = wu.random_table(rng, bd)
    cases, body = [], bytearray()
    head = np.array([bd, signal], np.int32).tobytes() + np.array([cw, dw[1], dw[2]], np.float64).tobytes() + lut.tobytes()
    cfs = {1: (1, 1), 2: (1, 0), 3: (0, 0)}   # ChromaFormat 420 / 422 / 444
    for (w, h) in [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (2, 2), (2, 8), (6, 4), (12, 8), (24, 16), (48, 32)]:
        for comp in (0, 1, 2):
            cf = int(rng.integers(1, 4))
            sx, sy = cfs[cf] if comp else (0, 0)
            org, cur, luma = _block(rng, bd, w, h, comp, sx, sy)
            lb = luma if comp else np.zeros((0, 0), np.int16)
            body += np.array([w, h, comp, cf, lb.shape[1], lb.shape[0]], np.int32).tobytes() + org.tobytes() + cur.tobytes() + lb.tobytes()
            raw = wu.sse_wtd(org, cur, comp, lut, signal, cw, luma, sx, sy)
            cases.append(raw if comp == 0 else int(dw[comp] * raw))   # RdCost.cpp:448-451: fp64 product, truncated
    inp = tmp_path / "in.bin"
    inp.write_bytes(head + np.array([len(cases)], np.int32).tobytes() + bytes(body))
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split()
    assert lines[-1] == "applyWeight-fallback-ok"
    assert [int(v) for v in lines[:-1]] == cases
