"""Records tests/golden/lfnst_mode.npz from the REAL reference: for each of the 25 luma shapes 4 .. 64 x 4 .. 64 and every regular mode 0 .. 66 the wide-angle mode
of PU::getWideAngle, g_lfnstLut[ TrQuant::getLFNSTIntraMode( . ) ] and TrQuant::getTransposeFlag( . ), driven by the small helper tests/golden/gen_lfnst_mode_ref.cpp
(the project's own text) -- the two TrQuant members are the reference's own, called on a default-constructed TrQuant, not restatements -- and the table g_lfnstLut
itself.  The helper is built here by hand against the reference headers and oracle/_ref/libvtmref.so (make -f oracle/Makefile.ref first); it is not part of the build
and never runs on a GPU machine:

    python tests/golden/gen_lfnst_mode_golden.py

The file holds `lut` (g_lfnstLut whole, uint8), `shapes` (25 x (w, h)) and `modes` (25 x 67 x (wide-angle mode, set index, transpose flag), int32)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import oracle_lib as ol     # noqa: E402

REF = "/root/reference/source"
HELPER = os.path.join(ROOT, "oracle", "_ref", "libgenlfnstmode.so")
SIDES = (4, 8, 16, 32, 64)


def build_helper():
    incs = ["-I%s/Lib" % REF, "-I%s/Lib/CommonLib" % REF, "-I%s/Lib/CommonLib/x86" % REF, "-I%s/Lib/libmd5" % REF, "-I%s/Lib/EncoderLib" % REF, "-I%s/Lib/Utilities" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-fPIC", "-shared", "-w", "-msse4.1", "-fno-access-control"] + incs +
                          [os.path.join(HERE, "gen_lfnst_mode_ref.cpp"), "-o", HELPER, "-L" + os.path.dirname(ol.REF_SO), "-lvtmref", "-Wl,-rpath,$ORIGIN"])
    L = C.CDLL(HELPER)
    L.gen_lfnst_lut.argtypes = [C.c_void_p]
    L.gen_lfnst_mode.argtypes = [C.c_int] * 3 + [C.c_void_p]
    return L


def main():
    L = build_helper()
    lut = np.zeros(256, np.uint8)
    n = L.gen_lfnst_lut(lut.ctypes.data)
    assert 95 <= n <= 256          # sizeof( g_lfnstLut ): indices 0 .. 94 are reachable from modes -14 .. 80
    lut = lut[:n].copy()
    shapes = [(w, h) for w in SIDES for h in SIDES]
    modes = np.zeros((len(shapes), 67, 3), np.int32)
    for s, (w, h) in enumerate(shapes):
        for mode in range(67):
            out = np.zeros(3, np.int32)
            L.gen_lfnst_mode(w, h, mode, out.ctypes.data)
            modes[s, mode] = out
    out = os.path.join(HERE, "lfnst_mode.npz")
    np.savez_compressed(out, lut=lut, shapes=np.array(shapes, np.int32), modes=modes)
    print("%s: %d shapes x 67 modes, wide-angle modes %d .. %d, %d bytes" % (out, len(shapes), modes[:, :, 0].min(), modes[:, :, 0].max(), os.path.getsize(out)))


if __name__ == "__main__":
    main()
