"""Records tests/golden/lmcs.npz from the REAL reference: AreaBuf<Pel>::scaleSignal, ::rspSignal and ::reconstruct (CommonLib/Buffer.cpp:399-464),
reached as strong symbols of oracle/_ref/libvtmref.so (tests/lmcs_util.RefLmcs).  Needs the reference build:

    python tests/golden/gen_lmcs_golden.py

scaleSignal: every case of lmcs_util.golden_case_inputs() (shapes 2x2 .. 16x16, 8 / 10 / 12 bits, both directions, nine scales, amplitudes 3, M and
32767 with samples at +-32767 and -32768) with its input and output block.  rspSignal / reconstruct: per bit depth a forward LUT
(lmcs_util.make_lut), three blocks mapped through it and the clipped sums pred + resi.  Blocks are stored one after the other in flat int16
arrays; *_off[k] is the first sample of case k."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lmcs_util as lu      # noqa: E402
import oracle_lib as ol     # noqa: E402

RSP_SHAPES = [(4, 4), (8, 4), (16, 16)]   # (w, h)


def main():
    ref = lu.RefLmcs(ol.ref())
    ws, hs, bds, dirs, scales, off, ins, outs, pos = [], [], [], [], [], [], [], [], 0
    for w, h, bd, fwd, scale, blk in lu.golden_case_inputs():
        ws.append(w), hs.append(h), bds.append(bd), dirs.append(fwd), scales.append(scale), off.append(pos)
        ins.append(blk.reshape(-1)), outs.append(ref.scale_signal(blk, scale, fwd, bd).reshape(-1))
        pos += w * h
    rng = np.random.default_rng(77)
    r_w, r_h, r_bd, r_off, r_in, r_out, r_resi, r_reco, luts, pos = [], [], [], [], [], [], [], [], [], 0
    for bd in (8, 10, 12):
        lut = lu.make_lut(100 + bd, bd)
        luts.append(np.concatenate([lut, np.zeros(4096 - lut.size, np.int16)]))
        for (w, h) in RSP_SHAPES:
            blk = rng.integers(0, 1 << bd, (h, w)).astype(np.int16)
            blk[0, 0], blk[h - 1, w - 1] = 0, (1 << bd) - 1
            resi = rng.integers(-(1 << bd), (1 << bd) + 1, (h, w)).astype(np.int16)
            mapped = ref.rsp_signal(blk, lut)
            r_w.append(w), r_h.append(h), r_bd.append(bd), r_off.append(pos)
            r_in.append(blk.reshape(-1)), r_out.append(mapped.reshape(-1)), r_resi.append(resi.reshape(-1))
            r_reco.append(ref.reconstruct(mapped, resi, bd).reshape(-1))
            pos += w * h
    out = os.path.join(HERE, "lmcs.npz")
    i8, i16 = (lambda a: np.array(a, np.int8)), (lambda a: np.array(a, np.int16))
    np.savez_compressed(out, sc_w=i8(ws), sc_h=i8(hs), sc_bd=i8(bds), sc_dir=i8(dirs), sc_scale=i16(scales), sc_off=np.array(off, np.int32),
                        sc_in=np.concatenate(ins), sc_out=np.concatenate(outs), rsp_w=i8(r_w), rsp_h=i8(r_h), rsp_bd=i8(r_bd), rsp_off=np.array(r_off, np.int32),
                        rsp_in=np.concatenate(r_in), rsp_out=np.concatenate(r_out), rsp_resi=np.concatenate(r_resi), rsp_reco=np.concatenate(r_reco),
                        rsp_lut=np.stack(luts))
    print("%s: %d + %d cases, %d bytes" % (out, len(ws), len(r_w), os.path.getsize(out)))


if __name__ == "__main__":
    main()
