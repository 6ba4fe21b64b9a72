"""Generates tests/golden/wp.npz: weighted distortions (RdCostWeightPrediction::xGetSADw / xGetSSEw / xGetHADsw) and weighted sample ops
(WeightPrediction::addWeightUni / addWeightBi) computed by the REAL reference (oracle/_ref/libvtmref.so) on seeded inputs.

    python tests/golden/gen_wp_golden.py

Distortion cases d_*: kind, w, h, bd, bi, wp = (w, offset, shift, round), maxDist, org / cur offsets into `org` / `cur`, the reference's value.
Sample-op cases p_*: mode, w, h, bd, wp = (w0, w1, offset, shift, round), src0 / src1 / dst offsets into `src` / `dst`, dst = the reference's output."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_lib  # noqa: E402
import wp_util as wu  # noqa: E402

WP_UNI, WP_BI = 0, 1


def main():
    ref = wu.RefWP(oracle_lib.ref())
    rng = np.random.default_rng(2026)
    org, cur, d = [], [], {k: [] for k in ("kind", "w", "h", "bd", "bi", "wp", "max", "org_off", "cur_off", "dist")}
    no = nc = 0
    shapes = {wu.SAD: wu.SAD_SHAPES, wu.SSE: wu.SSE_SHAPES, wu.SATD: wu.HAD_SHAPES}
    for kind in (wu.SAD, wu.SATD, wu.SSE):
        for bd in (8, 10, 12):
            for bi in (0, 1):
                for (w, h) in shapes[kind]:
                    for wide in (False, True):
                        o, c = wu.random_block(rng, w, h, bd, bi, wide)
                        org.append(o.reshape(-1))
                        cur.append(c.reshape(-1))
                        wps = [wu.random_wp(rng, bd), wu.derive_uni(1 << 2, int(rng.choice([0, 127, -128])), 2, bd), wu.derive_uni(-90, 7, 0, bd)]
                        for wp in wps:
                            cuts = wu.max_dist_cuts(wu.sad_rows(o, c, wp, bd, bi)) if kind == wu.SAD else [wu.U64]
                            for md in cuts:
                                for k, v in (("kind", kind), ("w", w), ("h", h), ("bd", bd), ("bi", bi), ("wp", wp), ("max", md), ("org_off", no),
                                             ("cur_off", nc), ("dist", ref.dist(kind, o, c, wp, bd, bi, md))):
                                    d[k].append(v)
                        no += o.size
                        nc += c.size
    src, dst, p = [], [], {k: [] for k in ("mode", "w", "h", "bd", "wp", "src0_off", "src1_off", "dst_off")}
    ns = nd = 0
    for bd in (8, 10, 12):
        for (w, h) in [(4, 4), (8, 8), (16, 16), (12, 8), (3, 5), (2, 8), (64, 4), (128, 2)]:
            for ld in (0, 1, 3, 7):
                s0 = rng.integers(-8192, 24576, (h, w)).astype(np.int16)
                s1 = rng.integers(-8192, 24576, (h, w)).astype(np.int16)
                src += [s0.reshape(-1), s1.reshape(-1)]
                for w0, io0 in [(1 << ld, 0), (1 << ld, int(rng.integers(-128, 128))), (int(rng.integers(-128, 128)), int(rng.choice([-128, 127])))]:
                    u = wu.derive_uni(w0, io0, ld, bd)
                    b = wu.derive_bi(w0, io0, int(rng.integers(-128, 128)), int(rng.integers(-128, 128)), ld, bd)
                    for mode, wp, out in ((WP_UNI, (u[0], 0, u[1], u[2], u[3]), ref.add_weight_uni(s0, u[0], u[1], u[2], bd)),
                                          (WP_BI, b, ref.add_weight_bi(s0, s1, *b[:4], bd))):
                        dst.append(out.reshape(-1))
                        for k, v in (("mode", mode), ("w", w), ("h", h), ("bd", bd), ("wp", wp), ("src0_off", ns), ("src1_off", ns + w * h),
                                     ("dst_off", nd)):
                            p[k].append(v)
                        nd += w * h
                ns += 2 * w * h
    out = dict(org=np.concatenate(org).astype(np.int16), cur=np.concatenate(cur).astype(np.int16), src=np.concatenate(src).astype(np.int16),
               dst=np.concatenate(dst).astype(np.int16))
    for k, v in d.items():
        out["d_" + k] = np.array(v, np.uint64 if k in ("max", "dist") else np.int64)
    for k, v in p.items():
        out["p_" + k] = np.array(v, np.int64)
    path = os.path.join(HERE, "wp.npz")
    np.savez_compressed(path, **out)
    print(path, len(d["dist"]), "distortions", len(p["mode"]), "sample-op blocks", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
