"""Writes tests/golden/sse_wtd.npz: DF_SSE*_WTD distortions computed by the REAL reference (oracle/_ref/libvtmref.so, RdCost::getWeightedMSE summed
over the block as RdCost::xGetSSE*_WTD does, reference CommonLib/RdCost.cpp:3055-3463) on seeded blocks.  Run after build():

    python tests/golden/gen_wtd_golden.py

Covers every slot width (2 .. 128 and the non-powers 6 / 12 / 24 / 48), Y and Cb / Cr under 4:2:0 / 4:2:2 / 4:4:4, 8 / 10 / 12-bit, SDR (chroma by
m_chromaWeight) and PQ (chroma by the co-located luma level, the reference's own PQ table).  Layout:
    lut<k>, set_bd, set_signal, set_chroma     the weight-table sets
    c_set, c_w, c_h, c_comp, c_csx, c_csy      one row per block
    c_org_off, c_cur_off, c_luma_off, c_luma_stride, c_dist
    org, cur, luma                             int16 sample pools (org / cur stride = width)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_lib  # noqa: E402
import wtd_util as wu  # noqa: E402

WIDTHS = (2, 4, 8, 16, 32, 64, 128, 6, 12, 24, 48)


def heights(w):
    return (2, 4) if w >= 128 else (2, 8) if w >= 64 else (4, 16) if w >= 16 else (2, 8)


def main():
    ref = wu.RefWeightedMSE(oracle_lib.ref())
    rng = np.random.default_rng(2024)
    out, sets, rows = {}, [], []
    pools = {"org": [], "cur": [], "luma": []}
    size = {"org": 0, "cur": 0, "luma": 0}

    def put(name, a):
        off = size[name]
        pools[name].append(np.ascontiguousarray(a, np.int16).reshape(-1))
        size[name] += a.size
        return off

    for bd in (8, 10, 12):
        for signal in (wu.SDR, wu.PQ):
            cw = float(rng.uniform(0.5, 2.0))
            if signal == wu.PQ:
                ref.set_state(bd, signal, cw)              # the reference builds its own PQ table
                lut = ref.table(bd)
            else:
                lut = wu.random_table(rng, bd)
                ref.set_state(bd, signal, cw, lut)
            k = len(sets)
            out["lut%d" % k] = lut
            sets.append((bd, signal, cw))
            mx = 1 << bd
            for w in WIDTHS:
                for h in heights(w):
                    cases = [(0, 0, 0)] + [(c, sx, sy) for (sx, sy) in wu.CF_SCALE.values() for c in (1, 2)]
                    for comp, sx, sy in cases:
                        if comp and (rng.random() < 0.5):   # half of the chroma (format, component) pairs per size: keeps the file small
                            continue
                        org = rng.integers(0, mx, (h, w))
                        cur = np.clip(org + rng.integers(-mx // 4, mx // 4 + 1, (h, w)), 0, mx - 1)
                        luma = rng.integers(0, mx, (h << sy, ((w - 1) << sx) + 1)) if comp else np.zeros((1, 1), np.int64)
                        dist = ref.block(org, cur, comp, luma if comp else None, sx, sy)
                        rows.append((k, w, h, comp, sx, sy, put("org", org), put("cur", cur), put("luma", luma), luma.shape[1], dist))
    out["set_bd"] = np.array([s[0] for s in sets], np.int32)
    out["set_signal"] = np.array([s[1] for s in sets], np.int32)
    out["set_chroma"] = np.array([s[2] for s in sets], np.float64)
    cols = ["c_set", "c_w", "c_h", "c_comp", "c_csx", "c_csy", "c_org_off", "c_cur_off", "c_luma_off", "c_luma_stride"]
    for i, c in enumerate(cols):
        out[c] = np.array([r[i] for r in rows], np.int64)
    out["c_dist"] = np.array([r[-1] for r in rows], np.uint64)
    for name in pools:
        out[name] = np.concatenate(pools[name])
    path = os.path.join(HERE, "sse_wtd.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d blocks, %d bytes" % (path, len(rows), os.path.getsize(path)))


if __name__ == "__main__":
    main()
