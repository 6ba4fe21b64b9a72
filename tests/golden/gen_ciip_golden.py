"""Records tests/golden/ciip.npz from the REAL reference, driven by the small helper tests/golden/gen_ciip_ref.cpp (the project's own text): per case and component
(Y, Cb, Cr of a 4:2:0 CU) what initPredIntraParams + xFilterReferenceSamples + predIntraAng leave under pu.ciipFlag (planar luma, DM_CHROMA chroma) from lines
chosen here, and what IntraPrediction::geneWeightedPred leaves for a random inter block.  The CU lives in a real CodingStructure with an optional left and above
neighbour CU, each inter or intra, so the weights come from the reference's own getPURestricted / CU::isIntra.  The one step of initIntraPatternChType that is not
run is the fetch of the lines from a picture (xFillReferenceSamples): the lines are placed where it would have left them, as gen_isp_ref.cpp does.

The helper is built here by hand against the reference headers and oracle/_ref/libvtmref.so (make -f oracle/Makefile.ref first); it is not part of the build and
never runs on a GPU machine:

    python tests/golden/gen_ciip_golden.py

Cases: luma shapes 16x4, 4x16, 8x8, 32x8, 16x16 with every neighbour combination (absent, inter, intra on each side), 64x64 with one combination per weight; 8, 10
and 12 bit and the two kinds of lines (flat; random at full range) rotate through the cases of a shape.  A chroma block of width 2 (4x16) is not recorded: the
reference leaves the inter chroma there."""
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
import oracle_lib as ol     # noqa: E402

REF = "/root/reference/source"
HELPER = os.path.join(ROOT, "oracle", "_ref", "libgenciip.so")
SHAPES = [(16, 4), (4, 16), (8, 8), (32, 8), (16, 16), (64, 64)]
ALL_NEIGHBOURS = [(l, a) for l in range(3) for a in range(3)]      # 0 absent, 1 inter, 2 intra
LARGE_NEIGHBOURS = [(0, 1), (2, 0), (2, 2)]                        # one per weight


def build_helper():
    incs = ["-I%s/Lib" % REF, "-I%s/Lib/CommonLib" % REF, "-I%s/Lib/CommonLib/x86" % REF, "-I%s/Lib/libmd5" % REF, "-I%s/Lib/EncoderLib" % REF, "-I%s/Lib/Utilities" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-fPIC", "-shared", "-w", "-msse4.1", "-fno-access-control"] + incs +
                          [os.path.join(HERE, "gen_ciip_ref.cpp"), "-o", HELPER, "-L" + os.path.dirname(ol.REF_SO), "-lvtmref", "-Wl,-rpath,$ORIGIN"])
    L = C.CDLL(HELPER)
    L.gen_ciip_case.argtypes = [C.c_int] * 5 + [C.c_void_p] * 5
    return L


def record(L, rng):
    cases, lines, inters, intras, blends, infos = [], [], [], [], [], []
    for si, (w, h) in enumerate(SHAPES):
        for k, (lk, ak) in enumerate(LARGE_NEIGHBOURS if w * h > 1024 else ALL_NEIGHBOURS):
            bd, kind = (8, 10, 12)[(k + si) % 3], (k // 3 + si) & 1           # kind 0: flat, 1: random at full range
            comp = [(w, h), (w // 2, h // 2), (w // 2, h // 2)]
            ln = [np.concatenate(iu.make_lines(rng, cw, ch, 0, bd, "random" if kind else "const")) for cw, ch in comp]
            it = [rng.integers(0, 1 << bd, (ch, cw)).astype(np.int16) for cw, ch in comp]
            ia = [np.zeros((ch, cw), np.int16) for cw, ch in comp]
            bl = [np.zeros((ch, cw), np.int16) for cw, ch in comp]
            info = np.zeros(3, np.int32)
            ptr = lambda arrs: (C.c_void_p * 3)(*[a.ctypes.data for a in arrs])      # noqa: E731
            assert L.gen_ciip_case(w, h, bd, lk, ak, ptr(ln), ptr(it), ptr(ia), ptr(bl), info.ctypes.data) == 0
            cases.append((w, h, bd, lk, ak, kind))
            infos.append(info)
            for c, (cw, ch) in enumerate(comp):
                if cw == 2:
                    assert info[c] == -1
                    continue
                lines.append(ln[c]); inters.append(it[c].reshape(-1)); intras.append(ia[c].reshape(-1)); blends.append(bl[c].reshape(-1))    # noqa: E702
    return dict(cases=np.array(cases, np.int32), info=np.concatenate(infos), lines=np.concatenate(lines).astype(np.int16), inter=np.concatenate(inters),
                intra=np.concatenate(intras), blend=np.concatenate(blends))


def save_npz(path, data):
    """an .npz with fixed member dates, so that a second recording is the same file byte for byte"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(data):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(data[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def main():
    L = build_helper()
    data = record(L, np.random.default_rng(2026))
    out = os.path.join(HERE, "ciip.npz")
    save_npz(out, data)
    print("%s: %d cases, %d bytes" % (out, len(data["cases"]), os.path.getsize(out)))


if __name__ == "__main__":
    main()
