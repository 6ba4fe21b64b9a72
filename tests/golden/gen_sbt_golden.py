"""Records tests/golden/sbt.npz from the REAL reference through tests/sbt_util.RefSbt: TrQuant::xT, Quant::quant / dequant and TrQuant::xIT with the mtsIdx
of the SBT transform pair for the sub-TU chain, RdCost::xGetSSE (ref_dist) for the SSE of the coded tile and for the partition sums of
InterSearch::calcMinDistSbt.  Needs the reference build (make -f oracle/Makefile.ref):

    python tests/golden/gen_sbt_golden.py

Per case of sbt_util.golden_case_inputs() -- every CU shape of GOLDEN_SHAPES x every allowed mode, on the luma block and on the CU's 4:2:0 chroma block; bit
depth, QP and slice type rotate -- the file holds (w, h, mode, luma, bd, qp, irap), the component's residual block, the real members' levels, the dequantised
and inverse-transformed sub-TU, its SSE and absSum, and the 4 x 4 partition SSEs of the residual against zero.  Blocks lie one after the other in flat arrays:
off[k] is the first sample of case k's residual, sub_off[k] that of its sub-TU arrays."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_lib as ol     # noqa: E402
import sbt_util as su       # noqa: E402


def main():
    ref = su.RefSbt(ol.ref())
    meta = {k: [] for k in ("w", "h", "mode", "luma", "bd", "qp", "irap", "off", "sub_off", "sse", "abs_sum")}
    resi, levels, rec, part, pos, sub_pos = [], [], [], [], 0, 0
    for w, h, mode, luma, bd, qp, irap, r in su.golden_case_inputs():
        e = ref.chain(r, su.idx_from_mode(mode), su.pos_from_mode(mode), luma, bd, qp, irap)
        for k, v in zip(("w", "h", "mode", "luma", "bd", "qp", "irap", "off", "sub_off", "sse", "abs_sum"), (w, h, mode, luma, bd, qp, irap, pos, sub_pos, e["sseCoded"], e["absSum"])):
            meta[k].append(v)
        resi.append(r.reshape(-1)), levels.append(e["levels"]), rec.append(e["rec_sub"].reshape(-1))
        part.append(ref.part_sums(r, np.zeros_like(r), su.num_part(w), su.num_part(h), bd))
        pos += r.size
        sub_pos += e["levels"].size
    out = os.path.join(HERE, "sbt.npz")
    i8, i32 = (lambda a: np.array(a, np.int8)), (lambda a: np.array(a, np.int32))
    np.savez_compressed(out, w=i8(meta["w"]), h=i8(meta["h"]), mode=i8(meta["mode"]), luma=i8(meta["luma"]), bd=i8(meta["bd"]), qp=i8(meta["qp"]), irap=i8(meta["irap"]),
                        off=i32(meta["off"]), sub_off=i32(meta["sub_off"]), sse=np.array(meta["sse"], np.uint64), abs_sum=i32(meta["abs_sum"]),
                        resi=np.concatenate(resi), levels=np.concatenate(levels).astype(np.int16), rec=np.concatenate(rec), part=np.array(part, np.uint64))
    print("%s: %d cases, %d bytes" % (out, len(meta["w"]), os.path.getsize(out)))


if __name__ == "__main__":
    main()
