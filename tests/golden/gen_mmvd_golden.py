"""Records tests/golden/mmvd.npz from the REAL reference: MergeCtx::setMmvdMergeCandiInfo (ContextModelling.cpp:355-528) for all 64 MMVD indices of a CU, driven by
the small helper tests/golden/gen_mmvd_ref.cpp (the project's own text) on a real PredictionUnit with a slice, its reference POC lists and pictures with longTerm
flags.  Per case and index: the motion it leaves (mv, refIdx, interDir), cu.BcwIdx as the list-1 weight, cu.imv == IMV_HPEL and
PU::isBiPredFromDifferentDirEqDistPoc.

The helper is built here by hand against the reference headers and oracle/_ref/libvtmref.so (make -f oracle/Makefile.ref first); it is not part of the build and
never runs on a GPU machine:

    python tests/golden/gen_mmvd_golden.py

Cases, the product of: base kinds (list 0 only, list 1 only, bi); POC pairs (equal differences; opposite and equal distance; |d1| > |d0| and |d0| > |d1|, each on
one side and on opposite sides; a pair beyond the +-128 clip of getDistScaleFactor); long-term on neither picture / list 0 / list 1; disFracMmvd 0 / 1; base vectors
(zero, quarter, half and odd phases, one within 200 of +2^17 and one of -2^17 so that the storage clip engages -- two of them per case, as base 0 and base 1); CU
sizes 8x4, 4x8, 8x8, 16x16; BCW weights 4 and 10."""
import ctypes as C
import itertools
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
HELPER = os.path.join(ROOT, "oracle", "_ref", "libgenmmvd.so")
CUR_POC = 300
KINDS = [(0, -1), (-1, 0), (0, 0)]                      # refIdx pattern of base 0 (base 1 uses index 1 where base 0 uses 0)
POC_PAIRS = [(-2, -2), (-4, 4), (-1, -3), (-1, 3), (5, 2), (5, -2), (-200, 150)]
LONG_TERM = [(0, 0), (1, 0), (0, 1)]
# (list-0 vector, list-1 vector) of base 0, then of base 1
MV_SETS = [(((0, 0), (0, 0)), ((4, -12), (-20, 8))),
           (((8, 24), (-8, 40)), ((5, -7), (13, 3))),
           ((((1 << 17) - 150, 37), (-(1 << 17) + 90, -61)), ((-(1 << 17) + 199, (1 << 17) - 3), ((1 << 17) - 1, -(1 << 17))))]
SIZES = [(8, 4), (4, 8), (8, 8), (16, 16)]
BCW = [4, 10]
BCW_WEIGHTS = (-2, 3, 4, 5, 10)


def build_helper():
    incs = ["-I%s/Lib" % REF, "-I%s/Lib/CommonLib" % REF, "-I%s/Lib/CommonLib/x86" % REF, "-I%s/Lib/libmd5" % REF, "-I%s/Lib/EncoderLib" % REF, "-I%s/Lib/Utilities" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-fPIC", "-shared", "-w", "-msse4.1", "-fno-access-control"] + incs +
                          [os.path.join(HERE, "gen_mmvd_ref.cpp"), "-o", HELPER, "-L" + os.path.dirname(ol.REF_SO), "-lvtmref", "-Wl,-rpath,$ORIGIN"])
    L = C.CDLL(HELPER)
    L.gen_mmvd_case.argtypes = [C.c_int] * 4 + [C.c_void_p] * 2
    return L


def main():
    L = build_helper()
    cases, outs = [], []
    for kind, pocs, lt, dis_frac, mvs, (w, h), bcw in itertools.product(KINDS, POC_PAIRS, LONG_TERM, (0, 1), MV_SETS, SIZES, BCW):
        base = np.zeros((2, 12), np.int32)
        for b in range(2):
            ref_idx = [r if r < 0 else b for r in kind]
            # base 1 mirrors the POC pair, so that both lists are the carrier once per case
            d = pocs if b == 0 else (pocs[1], pocs[0])
            t = lt if b == 0 else (lt[1], lt[0])
            base[b] = [mvs[b][0][0], mvs[b][0][1], mvs[b][1][0], mvs[b][1][1], ref_idx[0], ref_idx[1], CUR_POC + d[0], CUR_POC + d[1], t[0], t[1], (b + dis_frac) & 1,
                       BCW_WEIGHTS.index(bcw)]
        out = np.zeros((64, 10), np.int32)
        assert L.gen_mmvd_case(w, h, CUR_POC, dis_frac, base.ctypes.data, out.ctypes.data) == 0
        row = [w, h, dis_frac]
        for b in range(2):
            # the job's view of a base: vectors, refIdx, POC differences, longTerm, useAltHpelIf, the list-1 weight
            row += list(base[b, :6]) + [base[b, 6] - CUR_POC, base[b, 7] - CUR_POC] + list(base[b, 8:11]) + [bcw]
        cases.append(row)
        outs.append(out)
    outs = np.array(outs, np.int32)
    data = dict(cases=np.array(cases, np.int32), mv=outs[:, :, 0:4], small=outs[:, :, 4:].astype(np.int8))
    path = os.path.join(HERE, "mmvd.npz")
    np.savez_compressed(path, **data)
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
