"""Records tests/golden/cclm.npz from the REAL reference: IntraPrediction::initIntraPatternChType, xGetLumaRecPixels, xGetLMParameters, predIntraChromaLM and
initPredIntraParams / predIntraAng for Cb and Cr, driven by the small helper tests/golden/gen_cclm_ref.cpp (the project's own text) on a real Picture /
CodingStructure of 256 x 256 luma samples with 128 x 128 CTUs.  The helper is built here by hand against the reference headers and oracle/_ref/libvtmref.so
(make -f oracle/Makefile.ref first); it is not part of the build and never runs on a GPU machine:

    python tests/golden/gen_cclm_golden.py

Availability comes from where the CU lies (picture corner / edge, CTU row) and from the neighbouring CUs the helper adds and marks decoded; the file stores the
flags and counts the reference's own walks return.  Classes: none (picture corner), above only (left picture edge), left only (top picture edge), both, both with
partial and with full above-right / below-left, and both in the first row of a CTU.  The planes are cclm_util.hash_plane of a stored seed (random, alternating,
constant, and a nearly flat luma under alternating chroma), so the file holds no picture.  Per case: the header (cclm_util.golden_block), the four recorded lines,
the down-sampled luma of the LM and of the MDLM extent (inner, 2W top, 2H left; 0x5555 where the reference filled nothing), (a, b, shift) of 3 modes x 2
components, the LM predictions and the regular predictions of cclm_util.GOLDEN_REGULAR (every third of them above 256 samples)."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import cclm_util as cu      # noqa: E402
import oracle_lib as ol     # noqa: E402

REF = "/root/reference/source"
HELPER = os.path.join(ROOT, "oracle", "_ref", "libgencclm.so")
KINDS = ("random", "alt", "const", "swing")
CLASSES = ("none", "above", "left", "both", "partial", "full", "first_row")


class In(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("picW", "picH", "ctuSize", "bitDepth", "colocated", "x", "y", "w", "h", "numNbr")] + [("nbr", (C.c_int32 * 4) * 16), ("numModes", C.c_int32),
                                                                                                                              ("modes", C.c_int32 * 70)] + [(n, C.c_void_p) for n in ("luma", "cb", "cr")]


class Out(C.Structure):
    _fields_ = [("avail", C.c_int32 * 4), ("firstRow", C.c_int32)] + [(n, C.c_void_p) for n in ("lines", "dsLm", "dsMdlm", "params", "predLm", "predReg")]


def build_helper():
    incs = ["-I%s/Lib" % REF, "-I%s/Lib/CommonLib" % REF, "-I%s/Lib/CommonLib/x86" % REF, "-I%s/Lib/libmd5" % REF, "-I%s/Lib/EncoderLib" % REF, "-I%s/Lib/Utilities" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-fPIC", "-shared", "-w", "-msse4.1", "-fno-access-control"] + incs +
                          [os.path.join(HERE, "gen_cclm_ref.cpp"), "-o", HELPER, "-L" + os.path.dirname(ol.REF_SO), "-lvtmref", "-Wl,-rpath,$ORIGIN"])
    L = C.CDLL(HELPER)
    L.gen_cclm_case.argtypes = [C.POINTER(In), C.POINTER(Out)]
    return L


def placement(cls, lw, lh, k):
    """(x, y, neighbours) of a luma CU of lw x lh for an availability class"""
    if cls == "none":
        return 0, 0, []
    if cls == "above":
        return 0, 64, [(0, 0, lw * (1 + k % 2), 64)]
    if cls == "left":
        return 64, 0, [(0, 0, 64, lh * (1 + k % 2))]
    y = 128 if cls == "first_row" else 64
    aw, lhh = {"both": (lw, lh), "partial": (lw + max(4, lw // 2), lh + max(4, lh // 2) * (k % 2)), "full": (2 * lw, 2 * lh), "first_row": (2 * lw, lh)}[cls]
    return 64, y, [(0, y - 64, 64, 64), (64, y - 64, aw, 64), (0, y, 64, lhh)]


def main():
    L = build_helper()
    hdrs, lines, ds, params, preds, seen, k = [], [], [], [], [], collections.Counter(), 0
    for w, h in cu.SHAPES10:
        for cls in CLASSES:
            for coloc in (0, 1):
                bd, kind = (8, 10, 12)[k % 3], (k // 2 + k // 14) % 4
                if w * h > 256 and (k + coloc) % 2:       # the largest blocks alternate the collocated flag over the classes instead of taking both
                    k += 1
                    continue
                seed = 1000 + k
                luma, cb, cr = cu.golden_planes(seed, bd, KINDS[kind])
                x, y, nbrs = placement(cls, 2 * w, 2 * h, k)
                modes = cu.GOLDEN_REGULAR if w * h <= 256 else cu.GOLDEN_REGULAR[k % 3::3]
                i = In(cu.GOLDEN_PIC[0], cu.GOLDEN_PIC[1], cu.GOLDEN_CTU, bd, coloc, x, y, 2 * w, 2 * h, len(nbrs))
                for n, r in enumerate(nbrs):
                    i.nbr[n] = (C.c_int32 * 4)(*r)
                i.numModes = len(modes)
                i.modes = (C.c_int32 * 70)(*modes)
                i.luma, i.cb, i.cr = luma.ctypes.data, cb.ctypes.data, cr.ctypes.data
                ln, d_lm, d_md = np.zeros(2 * (2 * w + 2 * h + 2), np.int16), np.zeros(w * h + 2 * w + 2 * h, np.int16), np.zeros(w * h + 2 * w + 2 * h, np.int16)
                par, p_lm, p_rg = np.zeros(18, np.int32), np.zeros(6 * w * h, np.int16), np.zeros(2 * len(modes) * w * h, np.int16)
                o = Out()
                o.lines, o.dsLm, o.dsMdlm, o.params, o.predLm, o.predReg = (a.ctypes.data for a in (ln, d_lm, d_md, par, p_lm, p_rg))
                assert L.gen_cclm_case(C.byref(i), C.byref(o)) == 0
                above, left, ar, bl = (int(v) for v in o.avail)
                hdr = (w, h, bd, coloc, above, left, ar, bl, int(o.firstRow) and above, kind, x, y, seed)
                # which branches the case reaches (the numpy restatement, on the CPU)
                b = cu.golden_block(hdr, ln)
                for mode in cu.ALL_LM:
                    for c in (0, 1):
                        info = {}
                        cu.lm_params(b, c, mode, info=info)
                        for key, v in info.items():
                            seen[(key, int(np.sign(v))) if key in ("clamp", "a") else key] += 1
                hdrs.append(hdr + (len(modes),))
                lines.append(ln); ds += [d_lm, d_md]; params.append(par); preds += [p_lm, p_rg]
                k += 1
    for key in ("none", "diff0", ("clamp", 1), ("clamp", -1), ("a", -1), ("a", 1), "ar_clamp"):
        assert seen[key] >= 5, (key, seen)
    classes = collections.Counter((h[4], h[5], h[6] > 0, h[7] > 0, h[8]) for h in hdrs)
    out = os.path.join(HERE, "cclm.npz")
    np.savez_compressed(out, hdrs=np.array(hdrs, np.int32), lines=np.concatenate(lines), ds=np.concatenate(ds), params=np.array(params, np.int32), preds=np.concatenate(preds))
    assert os.path.getsize(out) < (1 << 20), os.path.getsize(out)
    print("%s: %d cases, %d bytes; branches %s; (above, left, ar, bl, firstRow) %s" % (out, len(hdrs), os.path.getsize(out), dict(seen), dict(classes)))


if __name__ == "__main__":
    main()
