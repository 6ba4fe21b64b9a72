"""Records tests/golden/isp.npz from the REAL reference.  Two parts:

1. The prediction side of intra sub-partitions, driven by the small helper tests/golden/gen_isp_ref.cpp (the project's own text): IntraPrediction::
   initPredIntraParams with cu->ispMode set, initIntraPatternChTypeISP for the regions behind the first -- on a reconstruction chosen here, in both availability
   branches (a real CodingStructure with or without a decomposed neighbour CU) -- and predIntraAng on every region.  Per case: the parameters of every region, the
   two lines every later region sees, the assembled prediction.
2. The transforms at the TU shapes only ISP has, through exports the reference library already has: ref_xT / ref_quant_dequant2 / ref_xIT at 1xN, 2xN, Nx1, Nx2
   (DCT2 on both sides, the pair of a side of 1 or 2) and with the DST7-DST7 index at the shapes with both sides in 4 .. 16; the mixed DCT2 / DST7 pairs per
   dimension through ref_fwd_trans / ref_inv_trans with the shifts and zero-out of TrQuant::xT / xIT.

The helper is built here by hand against the reference headers and oracle/_ref/libvtmref.so (make -f oracle/Makefile.ref first); it is not part of the build and
never runs on a GPU machine:

    python tests/golden/gen_isp_golden.py

Cases: every ISP CU shape up to 16x16 plus 4x64, 64x4, 32x32, 64x64, 8x32 and 32x8, both splits; modes 0, 1, 2, 18, 34, 50, 66, one wide angle per flat / tall
shape and two fractional slopes; both availability branches up to 16x16, alternating above.  Bit depth and the kind of lines rotate per shape."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import intra_util as iu     # noqa: E402
import isp_util as isp      # noqa: E402
import oracle_lib as ol     # noqa: E402

REF = "/root/reference/source"
HELPER = os.path.join(ROOT, "oracle", "_ref", "libgenisp.so")
MAX_LINE = 129
SMALL = [(4, 8), (8, 4), (4, 16), (16, 4), (8, 8), (8, 16), (16, 8), (16, 16)]
LARGE = [(4, 64), (64, 4), (32, 32), (64, 64), (8, 32), (32, 8)]
NARROW = [(1, 16), (2, 8), (2, 16), (16, 1), (8, 2), (16, 2), (1, 64), (64, 1), (2, 64)]
DST7_BOTH = [(4, 4), (8, 4), (4, 16), (16, 4), (16, 16), (8, 8)]
MIXED = [(2, 8), (8, 2), (2, 16), (16, 2), (8, 32), (32, 8), (64, 4), (4, 64), (16, 64), (64, 16), (2, 32), (32, 2)]


def build_helper():
    incs = ["-I%s/Lib" % REF, "-I%s/Lib/CommonLib" % REF, "-I%s/Lib/CommonLib/x86" % REF, "-I%s/Lib/libmd5" % REF, "-I%s/Lib/EncoderLib" % REF, "-I%s/Lib/Utilities" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-fPIC", "-shared", "-w", "-msse4.1", "-fno-access-control"] + incs +
                          [os.path.join(HERE, "gen_isp_ref.cpp"), "-o", HELPER, "-L" + os.path.dirname(ol.REF_SO), "-lvtmref", "-Wl,-rpath,$ORIGIN"])
    L = C.CDLL(HELPER)
    L.gen_isp_case.argtypes = [C.c_int] * 8 + [C.c_void_p] * 6
    return L


def modes_of(w, h):
    wide = [k for k in range(2, 67) if iu.wide_angle(w, h, k) != k]
    return [0, 1, 2, 18, 34, 50, 66, 7, 61] + ([wide[len(wide) // 2]] if wide else [])


def record_prediction(L, rng):
    blocks, cases, lines, recos, preds, params, next_lines = [], [], [], [], [], [], []
    for k, (w, h) in enumerate(SMALL + LARGE):
        bd, kind = (8, 10, 12)[k % 3], ("random", "random", "alt", "random", "const")[k % 5]
        top, left = iu.make_lines(rng, w, h, 0, bd, kind)
        reco = rng.integers(0, 1 << bd, (h, w)).astype(np.int16)
        blocks.append((w, h, bd))
        lines.append(np.concatenate([top, left]))
        recos.append(reco.reshape(-1))
        for split in (isp.HOR, isp.VER):
            g = isp.geometry(w, h, split)
            for mi, mode in enumerate(modes_of(w, h)):
                for avail in ((0, 1) if (w, h) in SMALL else ((mi + split) & 1,)):
                    nr = g["numRegions"]
                    pred, par, lo = np.zeros((h, w), np.int16), np.zeros(8 * nr, np.int32), np.zeros((max(nr - 1, 1), 2, MAX_LINE), np.int16)
                    assert L.gen_isp_case(w, h, mode, split, avail, bd, g["regW"], g["regH"], top.ctypes.data, left.ctypes.data, reco.ctypes.data, pred.ctypes.data,
                                          par.ctypes.data, lo.ctypes.data) == 0
                    par = par.reshape(nr, 8)
                    if mode < 2:
                        par[:, 2:4] = 0              # the member leaves the angle fields of planar / DC untouched
                    par[par[:, 2] <= 0, 4] = 0       # ... and angularScale of everything but positive angles
                    cases.append((len(blocks) - 1, mode, split, avail))
                    preds.append(pred.reshape(-1))
                    params.append(par.reshape(-1))
                    for r in range(1, nr):
                        next_lines += [lo[r - 1, 0, :w + g["regW"] + 1], lo[r - 1, 1, :h + g["regH"] + 1]]
    return dict(blocks=np.array(blocks, np.int32), cases=np.array(cases, np.int32), lines=np.concatenate(lines), recos=np.concatenate(recos), preds=np.concatenate(preds),
                params=np.concatenate(params), next_lines=np.concatenate(next_lines))


def record_transforms(rng):
    R = ol.ref()
    tr, tr_resi, tr_coef, tr_q, tr_dq, tr_rec = [], [], [], [], [], []
    for idx, (w, h, mts) in enumerate([(w, h, 0) for w, h in NARROW] + [(w, h, 2) for w, h in DST7_BOTH]):
        for bd in (8, 10, 12):
            qp, irap = (12, 27, 37, 51)[(idx + bd) % 4], idx & 1          # the base QP: QpParam adds the bit-depth offset
            resi = rng.integers(-(1 << bd) + 1, 1 << bd, (h, w)).astype(np.int16)
            coef, q, dq, s, rec = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), C.c_int32(), np.zeros((h, w), np.int16)
            assert R.ref_xT(ol.P(resi), w, w, h, bd, mts, ol.P(coef)) == 0
            assert R.ref_quant_dequant2(ol.P(coef), w, h, bd, qp, irap, mts, ol.P(q), C.byref(s), ol.P(dq)) == 0
            assert R.ref_xIT(ol.P(dq), w, h, bd, mts, ol.P(rec), w) == 0
            tr.append((w, h, bd, mts, qp, irap, s.value))
            tr_resi.append(resi.reshape(-1)); tr_coef.append(coef); tr_q.append(q); tr_dq.append(dq); tr_rec.append(rec.reshape(-1))    # noqa: E702
    mx, mx_resi, mx_coef, mx_in, mx_rec = [], [], [], [], []
    for idx, (w, h) in enumerate(MIXED):
        bd = (8, 10, 12)[idx % 3]
        th, tv = (isp.DST7 if 4 <= w <= 16 else isp.DCT2), (isp.DST7 if 4 <= h <= 16 else isp.DCT2)
        lw, lh, skw, skh = iu.flog2(w), iu.flog2(h), max(0, w - 32), max(0, h - 32)
        resi = rng.integers(-(1 << bd) + 1, 1 << bd, (h, w)).astype(np.int32)
        tmp, coef = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
        assert R.ref_fwd_trans(th, lw - 1, ol.P(resi), ol.P(tmp), lw + bd + 6 - 15, h, 0, skw) == 0
        assert R.ref_fwd_trans(tv, lh - 1, ol.P(tmp), ol.P(coef), lh + 6, w, skw, skh) == 0
        inp = np.clip(coef // 3, -32768, 32767).astype(np.int32)          # something a dequantiser could have left
        rec = np.zeros(w * h, np.int32)
        assert R.ref_inv_trans(tv, lh - 1, ol.P(inp), ol.P(tmp), 7, w, skw, skh, -32768, 32767) == 0
        assert R.ref_inv_trans(th, lw - 1, ol.P(tmp), ol.P(rec), 20 - bd, h, 0, skw, -32768, 32767) == 0
        mx.append((w, h, bd, th, tv))
        mx_resi.append(resi.reshape(-1).astype(np.int16)); mx_coef.append(coef); mx_in.append(inp); mx_rec.append(rec.astype(np.int16))    # noqa: E702
    return dict(tr=np.array(tr, np.int32), tr_resi=np.concatenate(tr_resi), tr_coef=np.concatenate(tr_coef), tr_q=np.concatenate(tr_q), tr_dq=np.concatenate(tr_dq),
                tr_rec=np.concatenate(tr_rec), mx=np.array(mx, np.int32), mx_resi=np.concatenate(mx_resi), mx_coef=np.concatenate(mx_coef), mx_in=np.concatenate(mx_in),
                mx_rec=np.concatenate(mx_rec))


def main():
    L = build_helper()
    rng = np.random.default_rng(2025)
    data = record_prediction(L, rng)
    data.update(record_transforms(rng))
    out = os.path.join(HERE, "isp.npz")
    np.savez_compressed(out, **data)
    print("%s: %d blocks, %d cases, %d + %d transform records, %d bytes" % (out, len(data["blocks"]), len(data["cases"]), len(data["tr"]), len(data["mx"]), os.path.getsize(out)))


if __name__ == "__main__":
    main()
