"""Records tests/golden/mip.npz from the REAL reference: MatrixIntraPrediction::prepareInputForPred and predBlock, driven by the small helper
tests/golden/gen_mip_ref.cpp (the project's own text), and the three trained matrices of CommonLib/MipData.h.  The helper is built here by hand against the
reference headers and oracle/_ref/libvtmref.so (make -f oracle/Makefile.ref first); it is not part of the build and never runs on a GPU machine:

    python tests/golden/gen_mip_golden.py

Cases: shapes up to 16 x 16 with every (mode, transposed) at 8, 10 and 12 bits (a block per depth); larger shapes with the first and the last mode in both
orientations, the bit depth rotating.  The kind of lines (random, alternating 0 / maximum, constant) rotates per block.  The file holds the matrices (m4x4, m8x8,
m16x16, flat uint8), per block (w, h, bd, offset of its lines) with top[0 .. w] then left[0 .. h] in `lines` (index 0 of both is unused: 0x7fff), per case (block,
mode, transposed, offset of its prediction in `preds`)."""
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
HELPER = os.path.join(ROOT, "oracle", "_ref", "libgenmip.so")
KINDS = ("random", "alt", "const")


def num_modes(w, h):
    return 16 if (w, h) == (4, 4) else 8 if (w == 4 or h == 4 or (w, h) == (8, 8)) else 6


def build_helper():
    incs = ["-I%s/Lib" % REF, "-I%s/Lib/CommonLib" % REF, "-I%s/Lib/CommonLib/x86" % REF, "-I%s/Lib/libmd5" % REF, "-I%s/Lib/EncoderLib" % REF, "-I%s/Lib/Utilities" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-fPIC", "-shared", "-w", "-msse4.1", "-fno-access-control"] + incs +
                          [os.path.join(HERE, "gen_mip_ref.cpp"), "-o", HELPER, "-L" + os.path.dirname(ol.REF_SO), "-lvtmref", "-Wl,-rpath,$ORIGIN"])
    L = C.CDLL(HELPER)
    L.gen_mip_case.argtypes = [C.c_int] * 5 + [C.c_void_p] * 3
    L.gen_mip_matrices.argtypes = [C.c_void_p] * 3
    return L


def main():
    L = build_helper()
    m4, m8, m16 = np.zeros(16 * 16 * 4, np.uint8), np.zeros(8 * 16 * 8, np.uint8), np.zeros(6 * 64 * 7, np.uint8)
    assert L.gen_mip_matrices(m4.ctypes.data, m8.ctypes.data, m16.ctypes.data) == 4736
    rng = np.random.default_rng(2025)
    blocks, cases, lines, preds, line_pos, pred_pos = [], [], [], [], 0, 0
    for k, (w, h) in enumerate(iu.SHAPES25):
        small, nm = w <= 16 and h <= 16, num_modes(w, h)
        for d, bd in enumerate((8, 10, 12) if small else ((8, 10, 12)[k % 3],)):
            top, left = iu.make_lines(rng, w, h, 0, bd, KINDS[(k + d) % 3])
            top, left = top[:w + 1].copy(), left[:h + 1].copy()
            top[0] = left[0] = iu.POISON
            blocks.append((w, h, bd, line_pos))
            lines += [top, left]
            line_pos += top.size + left.size
            jobs = [(m, t) for t in (0, 1) for m in range(nm)] if small else [(0, 0), (0, 1), (nm - 1, 0), (nm - 1, 1)]
            for mode, t in jobs:
                pred = np.zeros((h, w), np.int16)
                L.gen_mip_case(w, h, mode, t, bd, top.ctypes.data, left.ctypes.data, pred.ctypes.data)
                cases.append((len(blocks) - 1, mode, t, pred_pos))
                preds.append(pred.reshape(-1))
                pred_pos += w * h
    out = os.path.join(HERE, "mip.npz")
    np.savez_compressed(out, m4x4=m4, m8x8=m8, m16x16=m16, blocks=np.array(blocks, np.int32), cases=np.array(cases, np.int32), lines=np.concatenate(lines),
                        preds=np.concatenate(preds))
    print("%s: %d blocks, %d cases, %d bytes" % (out, len(blocks), len(cases), os.path.getsize(out)))


if __name__ == "__main__":
    main()
