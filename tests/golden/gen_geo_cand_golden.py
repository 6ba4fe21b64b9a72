"""Records tests/golden/geo_cand.npz from the REAL reference, driven by the small helper tests/golden/gen_geo_cand_ref.cpp (the project's own text): g_GeoParams,
g_weightOffset for all 64 x 4 x 4, the m_GeoModeTest order of a constructed EncCu and, per case, what the reference's own members leave for 14-bit candidate blocks
and an original chosen here: roundToOutputBitdepth, the whole-block and masked SADs (RdCost, DF_SAD_WITH_MASK; the walks over the reference's mask planes come from
geo_util.sad_walk), the list of a GeoComboCostList after its own sortByCost (the costs and the filter are formed here in numpy float64), the blended luma blocks of InterpolationFilter::xWeightedGeoBlk with their SATD and SAD, and blended Cb / Cr blocks of the first listed combinations.

The helper is built here by hand against the reference headers and oracle/_ref/libvtmref.so (make -f oracle/Makefile.ref first); it is not part of the build and
never runs on a GPU machine:

    python tests/golden/gen_geo_cand_golden.py

Cases: 8x8, 16x8, 8x16, 32x32, 64x16, 16x64, 64x64; 8, 10 and 12 bit; numCand 2, 3 and 6; per case the first lambda of LAMBDAS that gives the wanted list regime
(numPassed == 0, 0 < numPassed < 60, numPassed > 60).  A candidate block is the original plus small noise on one side of a line of its own and a shifted copy of
the original on the other, so that splits and pairs differ.  The reference's std::sort is not stable: a case is recorded only when no two costs among the first
min( numPassed, 61 ) list entries are equal (asserted), so that its order does not depend on the sort.  Blended luma blocks are kept for every listed combination
up to 256 samples per block and for the first three above, to keep the file small; the two distortions are kept for all."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import geo_util as gu       # noqa: E402
import oracle_lib as ol     # noqa: E402
from gen_ciip_golden import save_npz     # noqa: E402

REF = "/root/reference/source"
HELPER = os.path.join(ROOT, "oracle", "_ref", "libgengeocand.so")
# (w, h, bitDepth, numCand, regime): 0 numPassed == 0, 1 0 < numPassed < 60, 2 numPassed > 60
CASES = [(8, 8, 8, 2, 1), (8, 8, 10, 6, 2), (8, 8, 12, 3, 0), (16, 8, 10, 3, 2), (16, 8, 12, 2, 1), (8, 16, 8, 6, 2), (8, 16, 10, 2, 0), (32, 32, 10, 6, 2),
         (32, 32, 12, 2, 1), (64, 16, 8, 3, 1), (64, 16, 12, 6, 2), (16, 64, 10, 6, 2), (16, 64, 8, 3, 0), (64, 64, 10, 6, 2), (64, 64, 12, 3, 1)]
LAMBDAS = [0.37, 1.93, 4.71, 9.37, 17.53, 33.19, 57.61, 97.43, 181.07, 411.29, 1023.61, 4099.83, 65537.17, 0.0]
MAX_LIST = 1920


def build_helper():
    incs = ["-I%s/Lib" % REF, "-I%s/Lib/CommonLib" % REF, "-I%s/Lib/CommonLib/x86" % REF, "-I%s/Lib/libmd5" % REF, "-I%s/Lib/EncoderLib" % REF, "-I%s/Lib/Utilities" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-fPIC", "-shared", "-w", "-msse4.1", "-fno-access-control", "-ffp-contract=off"] + incs +
                          [os.path.join(HERE, "gen_geo_cand_ref.cpp"), "-o", HELPER, "-L" + os.path.dirname(ol.REF_SO), "-lvtmref", "-Wl,-rpath,$ORIGIN"])
    L = C.CDLL(HELPER)
    L.gen_geo_tables.argtypes = [C.c_void_p] * 3
    L.gen_geo_blend.argtypes = [C.c_int] * 5 + [C.c_void_p] * 3
    L.gen_geo_sads.argtypes = [C.c_int] * 4 + [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]
    L.gen_geo_sort.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.gen_geo_dist.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3
    return L


def make_blocks(rng, w, h, bd, num_cand):
    """the original and num_cand 14-bit blocks"""
    maxv, shift = (1 << bd) - 1, max(2, 14 - bd)
    yy, xx = np.mgrid[0:h, 0:w]
    org = (maxv / 2 + maxv / 4 * np.sin(xx / 3.1 + yy / 5.3) + rng.integers(-maxv // 16, maxv // 16 + 1, (h, w))).clip(0, maxv).astype(np.int64)
    preds = []
    for k in range(num_cand):
        ang = rng.uniform(0, 2 * np.pi)
        side = (xx - w / 2 + rng.uniform(-w / 4, w / 4)) * np.cos(ang) + (yy - h / 2 + rng.uniform(-h / 4, h / 4)) * np.sin(ang) > 0
        near = org + rng.integers(-2 - k, 3 + k, (h, w))
        far = np.roll(org, (1 + k, 2 + k), (0, 1)) + rng.integers(-maxv // 8, maxv // 8 + 1, (h, w))
        v = np.where(side, near, far).clip(0, maxv)
        preds.append(((v << shift) - 8192 + rng.integers(-(1 << (shift - 1)), 1 << (shift - 1), (h, w))).astype(np.int16))
    return org.astype(np.int16), preds


def run_sads(L, w, h, bd, num_cand, org, preds):
    """the reference's whole-block and masked SADs; the walks over its mask planes are geo_util.sad_walk's"""
    sw, sl = np.full(6, 2 ** 64 - 1, np.uint64), np.full(64 * 6, 2 ** 64 - 1, np.uint64)
    walk = np.array([gu.sad_walk(s, w, h) for s in range(64)], np.int32)
    ptr = (C.c_void_p * 6)(*[p.ctypes.data for p in preds] + [None] * (6 - num_cand))
    assert L.gen_geo_sads(w, h, bd, num_cand, org.ctypes.data, ptr, walk.ctypes.data, sw.ctypes.data, sl.ctypes.data) == 0
    return sw, sl


def run_case(L, w, h, bd, num_cand, lam, org, preds, sads):
    """the first pass in numpy float64 (side costs, the best whole-block cost, the filter, appended split by split in the pair order), the reference's own sort, and
    for the first 60 of the list the reference's blend and its two distortions"""
    sw, sl = sads
    large, lam = sl.reshape(64, 6), np.float64(lam)
    first = int(np.argmin(sw[:num_cand]))                            # the first strict minimum
    best = np.float64(int(sw[first])) + np.float64(first + 1) * lam
    rows, costs = [], []
    for s in range(64):
        for c0, c1 in gu.PAIRS[:num_cand * (num_cand - 1)]:
            t = (np.float64(int(large[s, c0])) + np.float64(c0 + 1) * lam) + (np.float64(int(sw[c1]) - int(large[s, c1])) + np.float64(c1 + 1) * lam)
            if t > best:
                continue
            rows.append((s, c0, c1))
            costs.append(t + np.float64(6) * lam)
    n = len(rows)
    lst, cost = np.array(rows, np.int32).reshape(n, 3).copy(), np.array(costs, np.float64)
    assert L.gen_geo_sort(n, lst.ctypes.data, cost.ctypes.data) == n
    blend, satd, sad = np.zeros((60, h, w), np.int16), np.zeros(60, np.uint64), np.zeros(60, np.uint64)
    for i in range(min(n, 60)):
        s, c0, c1 = lst[i].tolist()
        assert L.gen_geo_blend(w, h, bd, s, 0, preds[c0].ctypes.data, preds[c1].ctypes.data, blend[i].ctypes.data) == 0
        d = np.zeros(2, np.uint64)
        assert L.gen_geo_dist(w, h, bd, org.ctypes.data, blend[i].ctypes.data, d.ctypes.data) == 0
        satd[i], sad[i] = d
    return n, sw, sl, lst, cost, blend, satd, sad


def record(L, rng):
    params, offsets, order = np.zeros((64, 2), np.int16), np.zeros((64, 4, 4, 2), np.int16), np.zeros((30, 2), np.uint8)
    assert L.gen_geo_tables(params.ctypes.data, offsets.ctypes.data, order.ctypes.data) == 30
    d = dict(params=params, offsets=offsets, order=order)
    cases, lambdas, orgs, preds_all, sws, sls, lists, costs, blends, dists, cblends, cmeta, csrc = [], [], [], [], [], [], [], [], [], [], [], [], []
    for w, h, bd, num_cand, regime in CASES:
        found = None
        for attempt in range(20):
            org, preds = make_blocks(rng, w, h, bd, num_cand)
            sads = run_sads(L, w, h, bd, num_cand, org, preds)
            for lam in LAMBDAS:
                n, sw, sl, lst, cost, blend, satd, sad = run_case(L, w, h, bd, num_cand, lam, org, preds, sads)
                if (n == 0, 0 < n < 60, n > 60)[regime] and len(set(cost[:min(n, 61)].tolist())) == min(n, 61):
                    found = (lam, n, sw, sl, lst, cost, blend, satd, sad)
                    break
            if found:
                break
        assert found, (w, h, bd, num_cand, regime)
        lam, n, sw, sl, lst, cost, blend, satd, sad = found
        assert len(set(cost[:min(n, 61)].tolist())) == min(n, 61), "tie among the first list entries"      # the tie condition
        nt, nkeep = min(n, 60), min(n, 60) if w * h <= 256 else min(n, 3)
        cases.append((w, h, bd, num_cand, n, nkeep))
        lambdas.append(lam)
        orgs.append(org.reshape(-1))
        preds_all += [p.reshape(-1) for p in preds]
        sws.append(sw); sls.append(sl)                                                                      # noqa: E702
        lists.append(lst[:nt].reshape(-1)); costs.append(cost[:nt])                                         # noqa: E702
        blends.append(blend[:nkeep].reshape(-1))
        dists.append(np.stack([satd[:nt], sad[:nt]], 1).reshape(-1))
        # Cb and Cr of the first two listed combinations, from 14-bit chroma blocks chosen here
        for i in range(min(nt, 2)):
            for comp in (1, 2):
                shift = max(2, 14 - bd)
                s0 = ((rng.integers(0, 1 << bd, (h // 2, w // 2)) << shift) - 8192).astype(np.int16)
                s1 = ((rng.integers(0, 1 << bd, (h // 2, w // 2)) << shift) - 8192).astype(np.int16)
                out = np.zeros((h // 2, w // 2), np.int16)
                assert L.gen_geo_blend(w, h, bd, int(lst[i, 0]), comp, s0.ctypes.data, s1.ctypes.data, out.ctypes.data) == 0
                cmeta.append((len(cases) - 1, int(lst[i, 0]), comp))
                csrc += [s0.reshape(-1), s1.reshape(-1)]
                cblends.append(out.reshape(-1))
        print("%2dx%-2d %2d bit %d cand lambda %9.2f: %4d passed" % (w, h, bd, num_cand, lam, n))
    cat = lambda a, t: np.concatenate(a).astype(t) if a else np.zeros(0, t)      # noqa: E731
    d.update(cases=np.array(cases, np.int32), lambdas=np.array(lambdas, np.float64), org=cat(orgs, np.int16), pred=cat(preds_all, np.int16),
             sad_whole=np.stack(sws), sad_large=np.stack(sls), list=cat(lists, np.int32), cost=cat(costs, np.float64), blend=cat(blends, np.int16),
             dist=cat(dists, np.uint64), chroma_meta=np.array(cmeta, np.int32), chroma_src=cat(csrc, np.int16), chroma_blend=cat(cblends, np.int16))
    return d


def main():
    L = build_helper()
    data = record(L, np.random.default_rng(2026))
    out = os.path.join(HERE, "geo_cand.npz")
    save_npz(out, data)
    print("%s: %d cases, %d bytes" % (out, len(data["cases"]), os.path.getsize(out)))


if __name__ == "__main__":
    main()
