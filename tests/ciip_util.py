"""Combined inter-intra prediction (CIIP) restated in plain Python / numpy, following the flow of the reference's own text (the candidate loop EncCu.cpp:2460-2523,
IntraPrediction::geneWeightedPred IntraPrediction.cpp:682-722; the intra part through intra_util: xFilterReferenceSamples, xPredIntraPlanar and the PDPC of
predIntraAng).  It rests on no entry of the library: the tests compare vtmhip_ciip_host, vtmhip_ciip_blend_host and the device against it, and it against
tests/golden/ciip.npz.

A job is a dict: w, h, bd, left, above (the neighbour flags), lmcs, line_off, org_off, org_stride, cands = [cand ...]; a cand is a dict: mode (0 list 0, 1 list 1,
2 bi, 3 given), ref_off = [o0, o1], ref_stride = [s0, s1], mv = [[hor, ver], [hor, ver]], alt, src_off, src_stride, keep_off."""
import ctypes as C
import os

import numpy as np

import intra_util as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ciip.npz")
NO_COST = (1 << 64) - 1
L0, L1, BI, GIVEN = 0, 1, 2, 3
SIDES = (4, 8, 16, 32, 64)


def size_ok(w, h):
    """EncCu.cpp:2335-2339 on CU sides (powers of two from 4)"""
    return w in (4, 8, 16, 32, 64, 128) and h in (4, 8, 16, 32, 64, 128) and w * h >= 64 and w < 128 and h < 128


def num_cand(num_valid):
    return max(0, min(min(4, num_valid), 4))


def weight_intra(left, above):
    if left and above:
        return 3
    return 1 if not left and not above else 2


def planar(top, left, w, h, filt=True, pdpc=True):
    """the intra part: planar from the lines top (2w + 1) and left (2h + 1); filt: through the [1 2 1] filter (luma), pdpc: the planar PDPC on the same lines"""
    top, left = np.asarray(top, np.int64), np.asarray(left, np.int64)
    assert top.size == 2 * w + 1 and left.size == 2 * h + 1
    if filt:
        top, left = iu.filter_lines(top, left)
    pred = iu._planar(top, left, w, h)
    if pdpc and w >= 4 and h >= 4:
        scale = (iu.flog2(w) + iu.flog2(h) - 2) >> 2
        wl = 32 >> np.minimum(31, (np.arange(w) << 1) >> scale)
        for y in range(h):
            wt = 32 >> min(31, (y << 1) >> scale)
            val = pred[y]
            pred[y] = iu._pel(val + ((wl * (left[y + 1] - val) + wt * (top[1:w + 1] - val) + 32) >> 6))
    return pred.astype(np.int16)


def blend(inter, intra, w_intra):
    """geneWeightedPred: no clip"""
    return (((4 - w_intra) * inter.astype(np.int64) + w_intra * intra.astype(np.int64) + 2) >> 2).astype(np.int16)


def make_luts(bd):
    """a monotone, visibly non-linear forward LUT (a gamma curve with a knee) and its inverse (the smallest input that reaches the output)"""
    n = 1 << bd
    x = np.arange(n) / (n - 1.0)
    fwd = np.round((0.15 * x + 0.85 * x ** 0.6) * (n - 1)).astype(np.int64)
    fwd = np.maximum.accumulate(fwd)
    inv = np.searchsorted(fwd, np.arange(n), side="left").clip(0, n - 1)
    assert (np.diff(fwd) >= 0).all() and abs(int(fwd[n // 4]) - n // 4) > n // 8
    return fwd.astype(np.int16), inv.astype(np.int16)


def lut(table, block):
    return table[np.asarray(block, np.int64)]


def candidate(inter, intra, w_intra, fwd=None, inv=None):
    """-> (the blended block in the mapped domain, the block the distortion sees); fwd / inv: the LUT steps, each None to leave it out"""
    mapped = blend(inter if fwd is None else lut(fwd, inter), intra, w_intra)
    return mapped, (mapped if inv is None else lut(inv, mapped))


def make_cand(mode=L0, ref_off=(0, 0), ref_stride=(0, 0), mv=((0, 0), (0, 0)), alt=0, src_off=0, src_stride=0, keep_off=-1):
    return dict(mode=mode, ref_off=list(ref_off), ref_stride=list(ref_stride), mv=[list(mv[0]), list(mv[1])], alt=alt, src_off=src_off, src_stride=src_stride,
                keep_off=keep_off)


def make_job(w, h, bd, cands, left=0, above=0, lmcs=0, line_off=0, org_off=0, org_stride=None, num_cand=None):
    return dict(w=w, h=h, bd=bd, left=left, above=above, lmcs=lmcs, line_off=line_off, org_off=org_off, org_stride=w if org_stride is None else org_stride,
                cands=list(cands), num_cand=len(cands) if num_cand is None else num_cand)


def to_struct(job):
    from vtm_amd.lib import CiipJob
    j = CiipJob()
    j.lineOff, j.orgOff, j.orgStride, j.width, j.height, j.bitDepth = job["line_off"], job["org_off"], job["org_stride"], job["w"], job["h"], job["bd"]
    j.leftIntra, j.aboveIntra, j.lmcs, j.numCand = job["left"], job["above"], job["lmcs"], job["num_cand"]
    for k, c in enumerate(job["cands"][:4]):
        r = j.cand[k]
        r.mode, r.useAltHpelIf, r.srcOff, r.srcStride, r.keepOff = c["mode"], c["alt"], c["src_off"], c["src_stride"], c["keep_off"]
        for l in range(2):
            r.refOff[l], r.refStride[l], r.mv[l][0], r.mv[l][1] = c["ref_off"][l], c["ref_stride"][l], c["mv"][l][0], c["mv"][l][1]
    return j


def blend_struct(w, h, bd, line_off, pred_off, pred_stride, chroma=0, left=0, above=0, map_fwd=0):
    from vtm_amd.lib import CiipBlendJob
    j = CiipBlendJob()
    j.lineOff, j.predOff, j.predStride, j.width, j.height, j.bitDepth = line_off, pred_off, pred_stride, w, h, bd
    j.chroma, j.leftIntra, j.aboveIntra, j.mapFwd = chroma, left, above, map_fwd
    return j


def host_ciip(L, job, lines, org, inters, fwd=None, inv=None):
    """vtmhip_ciip_host -> (status, blended blocks [numCand][h][w], satd[4], sad[4])"""
    w, h, n = job["w"], job["h"], max(0, min(4, job["num_cand"]))
    keep = [np.ascontiguousarray(b, np.int16) for b in inters]
    ptrs = (C.c_void_p * 4)(*[b.ctypes.data for b in keep] + [None] * (4 - len(keep)))
    out = np.zeros((max(n, 1), h, w), np.int16)
    satd, sad = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
    lines, org = np.ascontiguousarray(lines, np.int16), np.ascontiguousarray(org, np.int16)
    st = L.vtmhip_ciip_host(C.byref(to_struct(job)), lines.ctypes.data, org.ctypes.data, ptrs, None if fwd is None else fwd.ctypes.data,
                            None if inv is None else inv.ctypes.data, out.ctypes.data, satd, sad)
    return st, out[:n], list(satd), list(sad)


def load_golden():
    """-> list of case dicts: w, h, bd, left_kind, above_kind (0 absent, 1 inter, 2 intra), kind, and per component c in 0 .. 2 (None where the chroma width is 2)
    lines, inter, intra, blend, info"""
    z = np.load(GOLDEN)
    cases, at = [], [0, 0]      # cursors into the line and the block pools
    for w, h, bd, lk, ak, kind in z["cases"]:
        case = dict(w=int(w), h=int(h), bd=int(bd), left_kind=int(lk), above_kind=int(ak), kind=int(kind), comp=[])
        for c in range(3):
            cw, ch = (w, h) if c == 0 else (w // 2, h // 2)
            if cw == 2:
                case["comp"].append(None)
                continue
            nl, nb = 2 * cw + 2 * ch + 2, cw * ch
            lines = z["lines"][at[0]:at[0] + nl]
            inter, intra, mixed = (z[k][at[1]:at[1] + nb].reshape(ch, cw) for k in ("inter", "intra", "blend"))
            at[0] += nl
            at[1] += nb
            case["comp"].append(dict(w=int(cw), h=int(ch), lines=lines, inter=inter, intra=intra, blend=mixed, info=int(z["info"][len(cases) * 3 + c])))
        cases.append(case)
    assert at[0] == z["lines"].size and at[1] == z["inter"].size
    return cases
