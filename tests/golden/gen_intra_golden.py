"""Records tests/golden/intra.npz from the REAL reference: IntraPrediction::initPredIntraParams, xFilterReferenceSamples and predIntraAng, driven by the small
helper tests/golden/gen_intra_ref.cpp (the project's own text; it places the chosen lines in the object's reference buffers).  The helper is built here by hand
against the reference headers and oracle/_ref/libvtmref.so (make -f oracle/Makefile.ref first); it is not part of the build and never runs on a GPU machine:

    python tests/golden/gen_intra_golden.py

Cases: blocks up to 16 x 16 with every mode (67 at multiRefIdx 0, 66 at 1 and 2); larger blocks with intra_util.boundary_modes() at multiRefIdx 0 and the fixed
modes at 1 or 2.  Bit depth (8 / 10 / 12) and the kind of lines (random, alternating 0 / maximum, constant) rotate per block.  The file holds, per block, (w, h, m,
bd) and its two lines; per case the block, the mode, the eight derived parameters (intra_util.PARAM_FIELDS order; angularScale as the member left it only where
the reference sets it -- positive angles -- and 0 elsewhere) and the prediction.  Lines and predictions lie one after the other in flat arrays."""
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
HELPER = os.path.join(ROOT, "oracle", "_ref", "libgenintra.so")


def build_helper():
    incs = ["-I%s/Lib" % REF, "-I%s/Lib/CommonLib" % REF, "-I%s/Lib/CommonLib/x86" % REF, "-I%s/Lib/libmd5" % REF, "-I%s/Lib/EncoderLib" % REF, "-I%s/Lib/Utilities" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-fPIC", "-shared", "-w", "-msse4.1", "-fno-access-control"] + incs +
                          [os.path.join(HERE, "gen_intra_ref.cpp"), "-o", HELPER, "-L" + os.path.dirname(ol.REF_SO), "-lvtmref", "-Wl,-rpath,$ORIGIN"])
    L = C.CDLL(HELPER)
    L.gen_intra_case.argtypes = [C.c_int] * 5 + [C.c_void_p] * 4
    return L


def main():
    L = build_helper()
    rng = np.random.default_rng(2024)
    blocks, cases, lines, preds, line_pos, pred_pos = [], [], [], [], 0, 0
    for k, (w, h) in enumerate(iu.SHAPES25):
        small = w <= 16 and h <= 16
        for m in (0, 1, 2) if small else (0, 1 + k % 2):
            bd, kind = (8, 10, 12)[(k + m) % 3], ("random", "alt", "random", "const")[(k + 2 * m) % 4]
            top, left = iu.make_lines(rng, w, h, m, bd, kind)
            modes = iu.modes_for(m) if small else iu.boundary_modes(w, h) if m == 0 else [1, 2, 18, 34, 50, 66]
            blocks.append((w, h, m, bd, line_pos))
            lines += [top, left]
            line_pos += top.size + left.size
            for mode in modes:
                pred, par = np.zeros((h, w), np.int16), np.zeros(9, np.int32)
                L.gen_intra_case(w, h, mode, m, bd, top.ctypes.data, left.ctypes.data, pred.ctypes.data, par.ctypes.data)
                assert par[8] == m
                if mode < 2:
                    par[2] = par[3] = 0          # the member leaves the angle fields of planar / DC untouched
                if mode < 2 or par[2] <= 0:
                    par[4] = 0                   # ... and angularScale of everything but positive angles
                cases.append((len(blocks) - 1, mode, pred_pos) + tuple(int(v) for v in par[:8]))
                preds.append(pred.reshape(-1))
                pred_pos += w * h
    out = os.path.join(HERE, "intra.npz")
    np.savez_compressed(out, blocks=np.array(blocks, np.int32), cases=np.array(cases, np.int32), lines=np.concatenate(lines), preds=np.concatenate(preds))
    print("%s: %d blocks, %d cases, %d bytes" % (out, len(blocks), len(cases), os.path.getsize(out)))


if __name__ == "__main__":
    main()
