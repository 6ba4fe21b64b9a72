"""Shared by test_geo_cand.py and test_gpu_geo_cand.py: the golden cases of tests/golden/geo_cand.npz, the reference's GEO tables restated in plain Python (the three
32-entry tables of the standard, the split list, g_weightOffset and the address arithmetic of xWeightedGeoBlk and of the masked SAD's set-up over the planes of
tests/golden/geo.npz), and the expectation of one CU built without libvtmhip: oracle functions for every sample step and the list in numpy float64."""
import ctypes as C
import os

import numpy as np

import oracle_lib as ol
from vtm_amd import lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "geo_cand.npz")
PLANES = os.path.join(HERE, "golden", "geo.npz")
NO_COST = 2 ** 64 - 1
M = 112                                                             # GEO_WEIGHT_MASK_SIZE
SHAPES = [(w, h) for w in (8, 16, 32, 64) for h in (8, 16, 32, 64) if w < 8 * h and h < 8 * w]

ANGLE2MASK = [0, -1, 1, 2, 3, 4, -1, -1, 5, -1, -1, 4, 3, 2, 1, -1, 0, -1, 1, 2, 3, 4, -1, -1, 5, -1, -1, 4, 3, 2, 1, -1]
ANGLE2MIRROR = [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2]
DIS = [8, 8, 8, 8, 4, 4, 2, 1, 0, -1, -2, -4, -4, -8, -8, -8, -8, -8, -8, -8, -4, -4, -2, -1, 0, 1, 2, 4, 4, 8, 8, 8]
# m_GeoModeTest, written out
PAIRS = [(0, 1), (1, 0), (0, 2), (1, 2), (2, 0), (2, 1), (0, 3), (1, 3), (2, 3), (3, 0), (3, 1), (3, 2), (0, 4), (1, 4), (2, 4), (3, 4), (4, 0), (4, 1), (4, 2), (4, 3),
         (0, 5), (1, 5), (2, 5), (3, 5), (4, 5), (5, 0), (5, 1), (5, 2), (5, 3), (5, 4)]


def split_params():
    """initGeoTemplate's list (Rom.cpp:703-718)"""
    out = []
    for a in range(32):
        for d in range(4):
            if (d == 0 and a >= 16) or (d in (0, 2) and ANGLE2MASK[a] in (0, 5)) or ANGLE2MASK[a] == -1:
                continue
            out.append((a, d))
    return out


SPLITS = split_params()


def weight_offset(split, w, h):
    """g_weightOffset (Rom.cpp:749-776)"""
    a, d = SPLITS[split]
    ox, oy = (M - w) >> 1, (M - h) >> 1
    if d > 0:
        if a % 16 == 8 or (a % 16 != 0 and h >= w):
            oy += (d * h) >> 3 if a < 16 else -((d * h) >> 3)
        else:
            ox += (d * w) >> 3 if a < 16 else -((d * w) >> 3)
    return ox, oy


def blend_walk(split, w, h, chroma):
    """xWeightedGeoBlk's walk (InterpolationFilter.cpp:923-956): plane index, first entry, step per sample, step per row (`width * stepX + stepY`)"""
    a = SPLITS[split][0]
    ox, oy = weight_offset(split, w, h)
    sc, mir = int(chroma), ANGLE2MIRROR[a]
    bw = w >> sc
    if mir == 2:
        step_x, step_y, first = 1 << sc, -((M << sc) + w), (M - 1 - oy) * M + ox
    elif mir == 1:
        step_x, step_y, first = -(1 << sc), (M << sc) + w, oy * M + (M - 1 - ox)
    else:
        step_x, step_y, first = 1 << sc, (M << sc) - w, oy * M + ox
    return ANGLE2MASK[a], first, step_x, bw * step_x + step_y


def sad_walk(split, w, h):
    """the masked SAD's set-up (EncCu.cpp:2924-2948): plane index, first entry, maskStride, stepX, maskStride2"""
    a = SPLITS[split][0]
    ox, oy = weight_offset(split, w, h)
    mir = ANGLE2MIRROR[a]
    if mir == 2:
        return ANGLE2MASK[a], (M - 1 - oy) * M + ox, -M, 1, -w
    if mir == 1:
        return ANGLE2MASK[a], oy * M + (M - 1 - ox), M, -1, w
    return ANGLE2MASK[a], oy * M + ox, M, 1, -w


def weight_planes():
    return np.ascontiguousarray(np.load(PLANES)["planes"])          # the six g_globalGeoWeights planes, recorded from the reference


def mask_planes():
    """g_globalGeoEncSADmask from the definition (Rom.cpp:730-745): weightIdx > 0, with weightIdx written out per plane entry"""
    out = np.zeros((6, M, M), np.int16)
    yy, xx = np.mgrid[0:M, 0:M]
    for a in range(9):
        if ANGLE2MASK[a] < 0:
            continue
        dx, dy = DIS[a], DIS[(a + 8) % 32]
        idx = (2 * (xx + 8) + 1) * dx + (2 * (yy + 8) + 1) * dy - ((dx << 7) + (dy << 7))
        out[ANGLE2MASK[a]] = idx > 0
    return out


def plane_block(plane, first, step_x, row_step, bw, bh):
    flat = plane.reshape(-1)
    yy, xx = np.mgrid[0:bh, 0:bw]
    return flat[first + yy * row_step + xx * step_x]


def load_golden():
    z = np.load(GOLDEN)
    out, po, pp, pl, pb, pd = [], 0, 0, 0, 0, 0
    for i, (w, h, bd, nc, n, nkeep) in enumerate(z["cases"].tolist()):
        nt, a = min(n, 60), w * h
        c = dict(w=w, h=h, bd=bd, num_cand=nc, num_passed=n, lam=float(z["lambdas"][i]), org=z["org"][po:po + a].reshape(h, w),
                 pred=[z["pred"][pp + k * a:pp + (k + 1) * a].reshape(h, w) for k in range(nc)], sad_whole=z["sad_whole"][i], sad_large=z["sad_large"][i].reshape(64, 6),
                 list=z["list"][pl * 3:(pl + nt) * 3].reshape(nt, 3), cost=z["cost"][pl:pl + nt], blend=z["blend"][pb:pb + nkeep * a].reshape(nkeep, h, w),
                 dist=z["dist"][pd:pd + 2 * nt].reshape(nt, 2), chroma=[])
        po += a; pp += nc * a; pl += nt; pb += nkeep * a; pd += 2 * nt                 # noqa: E702
        out.append(c)
    ps, pc = 0, 0
    for ci, split, comp in z["chroma_meta"].tolist():
        c = out[ci]
        a = (c["w"] // 2) * (c["h"] // 2)
        shp = (c["h"] // 2, c["w"] // 2)
        c["chroma"].append(dict(split=split, comp=comp, src0=z["chroma_src"][ps:ps + a].reshape(shp), src1=z["chroma_src"][ps + a:ps + 2 * a].reshape(shp),
                                blend=z["chroma_blend"][pc:pc + a].reshape(shp)))
        ps += 2 * a; pc += a                                                           # noqa: E702
    return dict(cases=out, params=z["params"], offsets=z["offsets"], order=z["order"])


def geo_job(w, h, bd, num_cand, lam, org_off=0, org_stride=None, cands=None):
    j = lib.GeoJob()
    j.orgOff, j.orgStride, j.width, j.height, j.bitDepth, j.numCand, j.sqrtLambda = org_off, org_stride or w, w, h, bd, num_cand, lam
    for k in range(6):
        j.cand[k].keepOff, j.cand[k].refStride = -1, w
    for k, (ref_off, ref_stride, mvx, mvy, keep) in enumerate(cands or []):
        j.cand[k].refOff, j.cand[k].refStride, j.cand[k].mv[0], j.cand[k].mv[1], j.cand[k].keepOff = ref_off, ref_stride, mvx, mvy, keep
    return j


def host_job(L, job, org, preds, use_satd=True, want_blend=True):
    """vtmhip_geo_host: (status, GeoResult, sadSplit 64 x 6, blend numTested x h x w)"""
    w, h = job.width, job.height
    keep = [np.ascontiguousarray(p, np.int16) for p in preds]
    ptr = (C.c_void_p * 6)(*[p.ctypes.data for p in keep] + [None] * (6 - len(keep)))
    res, split, blend = lib.GeoResult(), np.zeros((64, 6), np.uint64), np.zeros((60, max(h, 1), max(w, 1)), np.int16)
    org = np.ascontiguousarray(org, np.int16)
    st = L.vtmhip_geo_host(C.byref(job), org.ctypes.data, ptr, int(use_satd), C.byref(res), split.ctypes.data, blend.ctypes.data if want_blend else None)
    return st, res, split, blend


def result_rows(res):
    """the listed part of a GeoResult as tuples (splitDir, cand0, cand1, cost bits, dist)"""
    return [(c.splitDir, c.cand0, c.cand1, np.float64(c.cost).view(np.uint64).item(), c.dist) for c in res.combo]


def expect_sads(oracle, org, preds, w, h, bd, masks):
    """the rounded blocks' whole-block SADs and the 64 x numCand sadLarge: vo_sad, and vo_sad_mask over the mask planes with the reference's walk"""
    shift, maxv = max(2, 14 - bd), (1 << bd) - 1
    rounded = [np.ascontiguousarray(((p.astype(np.int64) + (1 << (shift - 1)) + 8192) >> shift).clip(0, maxv).astype(np.int16)) for p in preds]
    whole = [int(oracle.vo_sad(ol.P(org), w, ol.P(r), w, w, h, 0)) for r in rounded]
    large = np.full((64, 6), NO_COST, np.uint64)
    for s in range(64):
        mi, first, ms, sx, ms2 = sad_walk(s, w, h)
        for c in range(len(preds)):
            large[s, c] = oracle.vo_sad_mask(ol.P(org), w, ol.P(rounded[c]), w, w, h, 0, C.c_void_p(masks[mi].ctypes.data + 2 * first), ms, sx, ms2)
    return whole, large


def expect_list(whole, large, num_cand, lam, threshold_shift=0.0):
    """the filter and the order in numpy float64: rows (cost, splitDir, pair index), ascending by cost, then splitDir, then pair index"""
    lam = np.float64(lam)
    best_sad, best = None, None
    for c in range(num_cand):
        if best_sad is None or whole[c] < best_sad:
            best_sad, best = whole[c], np.float64(whole[c]) + np.float64(c + 1) * lam
    rows = []
    for s in range(64):
        for p in range(num_cand * (num_cand - 1)):
            c0, c1 = PAIRS[p]
            t = (np.float64(int(large[s, c0])) + np.float64(c0 + 1) * lam) + (np.float64(whole[c1] - int(large[s, c1])) + np.float64(c1 + 1) * lam)
            if t > best + np.float64(threshold_shift):
                continue
            rows.append((np.float64(t + np.float64(6) * lam), s, p))
    rows.sort(key=lambda r: (r[0], r[1], r[2]))
    return rows


def expect_cu(oracle, org, preds, w, h, bd, num_cand, lam, planes, masks, cap=60, threshold_shift=0.0, sads=None, walk=blend_walk):
    """One CU without libvtmhip.  org: the w x h original block; preds: 14-bit w x h blocks.  Every sample step is the oracle's (vo_sad, vo_sad_mask, and
    vo_weighted_geo_blk over the weight planes with the reference's walk, vo_satd and vo_sad: a row's last member is (satd, sad)); the costs, the filter and the order are numpy float64.
    cap / threshold_shift / walk: for the expectation check only."""
    maxv = (1 << bd) - 1
    org = np.ascontiguousarray(org, np.int16)
    whole, large = sads if sads is not None else expect_sads(oracle, org, preds, w, h, bd, masks)
    rows = expect_list(whole, large, num_cand, lam, threshold_shift)
    out, blends = [], []
    for cost, s, p in rows[:cap]:
        c0, c1 = PAIRS[p]
        mi, first, sx, row = walk(s, w, h, 0)
        got = np.zeros((h, w), np.int16)
        oracle.vo_weighted_geo_blk(ol.P(np.ascontiguousarray(preds[c0])), w, ol.P(np.ascontiguousarray(preds[c1])), w, ol.P(got), w, w, h,
                                   C.c_void_p(planes[mi].ctypes.data + 2 * first), sx, row, bd, 0, maxv)
        d = (int(oracle.vo_satd(ol.P(org), w, ol.P(got), w, w, h)), int(oracle.vo_sad(ol.P(org), w, ol.P(got), w, w, h, 0)))
        out.append((s, c0, c1, cost.view(np.uint64).item(), d))
        blends.append(got)
    return dict(whole=list(whole) + [NO_COST] * (6 - num_cand), large=large, num_passed=len(rows), rows=out, blends=blends)


def result_struct(e, use_satd=True):
    """the GeoResult the device must leave for expectation e (expect_cu), or for a skipped job (e is None)"""
    r = lib.GeoResult()
    for c in range(6):
        r.sadWhole[c] = NO_COST if e is None else e["whole"][c]
    for t in range(60):
        r.combo[t].dist = NO_COST
    if e is not None:
        r.numPassed, r.numTested = e["num_passed"], len(e["rows"])
        for t, (s, c0, c1, bits, d) in enumerate(e["rows"]):
            r.combo[t].splitDir, r.combo[t].cand0, r.combo[t].cand1, r.combo[t].dist = s, c0, c1, d[0 if use_satd else 1]
            r.combo[t].cost = np.uint64(bits).view(np.float64).item()
    return r
