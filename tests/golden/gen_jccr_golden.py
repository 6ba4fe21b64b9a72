"""Records tests/golden/jccr.npz from the REAL reference: the template instantiations fwdTransformCbCr<-3..3> / invTransformCbCr<-3..3>
(CommonLib/TrQuant.cpp:86-157), reached as weak symbols of oracle/_ref/libvtmref.so (tests/jccr_util.RefICT).  Needs the reference build:

    python tests/golden/gen_jccr_golden.py

Per case: (cb, cr, mode), the joint residual, the (d1, d2) pair and the component the inverse ICT rewrites when it runs on (cb, cr).  Blocks are
stored one after the other in flat int16 arrays; off[k] is the first sample of case k."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import jccr_util as ju      # noqa: E402
import oracle_lib as ol     # noqa: E402

SHAPES = [(2, 2), (2, 8), (4, 4), (8, 4), (4, 16), (16, 16), (8, 8), (16, 4), (2, 4), (8, 2)]   # (w, h)
AMPS = [3, 60, 1023, 32767]


def main():
    ref = ju.RefICT(ol.ref())
    rng = np.random.default_rng(20266)
    mode, ws, hs, off, dist = [], [], [], [], []
    cbs, crs, joints, invs = [], [], [], []
    pos = 0
    for m in ju.MODES:
        for (w, h) in SHAPES:
            for amp in AMPS:
                cb, cr = ju.random_pair(rng, w, h, amp, full_range=amp == 32767)
                if m == -2 and amp == 32767:
                    cb[0, 0], cb[h - 1, w - 1] = -32768, -32768      # the non-normative clip of invTransformCbCr<-2>
                joint, d = ref.fwd_ict(m, cb, cr)
                icb, icr = ref.inv_ict(m, cb, cr)
                mode.append(m), ws.append(w), hs.append(h), off.append(pos), dist.append(d)
                cbs.append(cb.reshape(-1)), crs.append(cr.reshape(-1))
                joints.append(np.zeros(w * h, np.int16) if joint is None else joint.reshape(-1))
                invs.append((icb if abs(m) == 3 else icr).reshape(-1))
                pos += w * h
    out = os.path.join(HERE, "jccr.npz")
    np.savez_compressed(out, mode=np.array(mode, np.int8), w=np.array(ws, np.int8), h=np.array(hs, np.int8), off=np.array(off, np.int32),
                        dist=np.array(dist, np.int64), cb=np.concatenate(cbs), cr=np.concatenate(crs), joint=np.concatenate(joints),
                        inv=np.concatenate(invs))
    print("%s: %d cases, %d bytes" % (out, len(mode), os.path.getsize(out)))


if __name__ == "__main__":
    main()
