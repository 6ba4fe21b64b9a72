"""Generates tests/golden/bd12.npz: 12-bit outputs of the REAL reference (oracle/_ref/libvtmref.so) for DMVR (xProcessDMVR, prediction and
pu.mvdL0SubPu), BDOF (xPredInterBlk(bioApplied) + applyBiOptFlow), motion compensation (xPredInterBlk uni / bi, addWeightedAvg at the default weight
= addAvg), the 2-D transforms (TrQuant::xT / xIT) and Quant::quant / dequant.

    python tests/golden/gen_bd12_golden.py

The pictures are not stored: they are synth.gen_frames( 256, 128, 3, seed=5, chroma=True ) at 12 bits (me_util.to_bit_depth), whose sums are
recorded in `plane_sums` so that a replay notices when the generator changes.  Per-case parameters are int32 rows (see the *_cols lists)."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import me_util  # noqa: E402
import oracle_lib as ol  # noqa: E402

BD, W, H, M = 12, 256, 128, 160
MTS_TYPES = {0: (0, 0), 2: (2, 2), 3: (1, 2), 4: (2, 1), 5: (1, 1)}


def planes():
    """Luma and both chroma planes of frames 0 and 2 at 12 bits, edge-padded by M (luma) / M / 2 (chroma): [list][comp] -> (padded array, origin offset, stride)."""
    from vtm_amd import synth
    fr = list(synth.gen_frames(W, H, 3, seed=5, chroma=True))
    out = []
    for f in (fr[0], fr[2]):
        row = []
        for c in range(3):
            m = M if c == 0 else M // 2
            p = np.ascontiguousarray(np.pad(me_util.to_bit_depth(f[c], BD), m, mode="edge"))
            row.append((p, m * p.shape[1] + m, p.shape[1]))
        out.append(row)
    return out, me_util.to_bit_depth(fr[1][0], BD)


def main():
    R = ol.ref()
    P, org = planes()
    rng = np.random.default_rng(1212)
    z = {"plane_sums": np.array([int(P[l][c][0].astype(np.int64).sum()) for l in range(2) for c in range(3)], np.int64)}
    at = lambda l, c, x=0, y=0: C.c_void_p(P[l][c][0].ctypes.data + 2 * (P[l][c][1] + y * P[l][c][2] + x))   # noqa: E731
    # DMVR: x, y, w, h, mv0h, mv0v, mv1h, mv1v, bio
    rows, pred, mvd = [], [], []
    for k in range(32):
        w, h = int(rng.choice([8, 16, 32])), int(rng.choice([8, 16, 32]))
        if w * h < 128:
            w = 16
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        base = np.array([48, 32]) + rng.integers(-40, 41, 2)
        mv = [int(-base[0]), int(-base[1]), int(base[0] + rng.integers(-24, 25)), int(base[1] + rng.integers(-24, 25))]
        if k % 5 == 0:
            mv[k % 4] &= ~15
        bio = k % 2
        nsub = (w // min(w, 16)) * (h // min(h, 16))
        e, d = np.zeros((h, w), np.int16), np.zeros(2 * 64, np.int32)
        R.ref_dmvr_pu(at(0, 0), at(1, 0), P[0][0][2], W, H, 128, x, y, w, h, *mv, BD, bio, ol.P(e), w, C.c_void_p(d.ctypes.data))
        rows.append([x, y, w, h, *mv, bio])
        pred.append(e.reshape(-1))
        mvd.append(d[:2 * nsub])
    z["dmvr"], z["dmvr_pred"], z["dmvr_mvd"] = np.array(rows, np.int32), np.concatenate(pred), np.concatenate(mvd)
    assert np.count_nonzero(z["dmvr_mvd"]) > 20
    # BDOF: x, y, w, h, mv0h, mv0v, mv1h, mv1v
    rows, pred = [], []
    for k in range(32):
        w, h = int(rng.choice([8, 16, 32])), int(rng.choice([8, 16, 32]))
        if w * h < 128:
            w = 16
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        mv = [int(v) for v in rng.integers(-500, 500, 4)]
        if k % 6 == 0:
            mv[k % 4] &= ~15
        e = np.zeros((h, w), np.int16)
        R.ref_bdof_pu(0, at(0, 0), at(1, 0), P[0][0][2], W, H, x, y, w, h, *mv, BD, ol.P(e), w)
        rows.append([x, y, w, h, *mv])
        pred.append(e.reshape(-1))
    z["bdof"], z["bdof_pred"] = np.array(rows, np.int32), np.concatenate(pred)
    # motion compensation: comp, x, y (luma units), w, h (of the plane), mode (0 / 1 uni list 0 / 1, 2 bi), mv0h, mv0v, mv1h, mv1v, alt half-sample filter
    rows, pred = [], []
    for k in range(60):
        comp = (0, 1, 2)[k % 3]
        lw, lh = int(rng.choice([8, 16, 32])), int(rng.choice([4, 8, 16, 32]))
        x, y = int(rng.integers(0, (W - lw) // 8 + 1)) * 8, int(rng.integers(0, (H - lh) // 8 + 1)) * 8
        mode, alt = k % 4 if k % 4 < 3 else 2, int(k % 7 == 0 and comp == 0)
        mv = [int(v) for v in rng.integers(-320, 320, 4)]
        if k % 5 == 0:
            mv[0] &= ~15
        w, h = (lw // 2, lh // 2) if comp else (lw, lh)
        p = []
        for l in ((0, 1) if mode == 2 else (mode,)):
            e = np.zeros((h, w), np.int16)
            R.ref_pred_inter_blk(comp, at(l, 0), P[l][0][2], at(l, max(comp, 1)), P[l][1][2] if comp != 2 else P[l][2][2], W, H, x, y, lw, lh,
                                 mv[2 * l], mv[2 * l + 1], int(mode == 2), BD, 3 if alt else 0, ol.P(e), w)
            p.append(e)
        if mode == 2:
            e = np.zeros((h, w), np.int16)
            R.ref_add_weighted_avg(ol.P(p[0]), w, ol.P(p[1]), w, ol.P(e), w, w, h, BD, 2)   # BCW index 2: weights 4 / 4, addAvg
            chk = np.zeros((h, w), np.int16)
            ol.oracle().vo_add_avg(ol.P(p[0]), w, ol.P(p[1]), w, ol.P(chk), w, w, h, BD)
            assert np.array_equal(chk, e)
            p = [e]
        rows.append([comp, x, y, w, h, mode, *mv, alt])
        pred.append(p[0].reshape(-1))
    z["mc"], z["mc_pred"] = np.array(rows, np.int32), np.concatenate(pred)
    # 2-D transforms: w, h, mtsIdx; residual, coefficients (xT), and xIT of the clipped coefficients
    rows, resi, coef, back = [], [], [], []
    for (w, h) in [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (4, 16), (16, 4), (8, 32), (32, 8), (64, 16), (16, 64)]:
        for mts in (0, 2, 3, 4, 5):
            if mts and max(w, h) > 32:
                continue
            th, tv = MTS_TYPES[mts]
            kinds = ("dc", "basis", "random") if w * h <= 1024 else ("dc", "basis")
            for kind in kinds:
                if kind == "dc":
                    r = np.full((h, w), 4095 if mts % 2 == 0 else -4095, np.int16)
                elif kind == "basis":
                    r = ol.basis_sign_block(w, h, th, tv, int(rng.integers(0, min(w, 32))), int(rng.integers(0, min(h, 32))), 4095)
                else:
                    r = rng.integers(-4095, 4096, (h, w)).astype(np.int16)
                c = np.zeros(w * h, np.int32)
                R.ref_xT(ol.P(r), w, w, h, BD, mts, ol.P(c))
                ci = np.clip(c, -32768, 32767).astype(np.int32)
                c2 = ci.reshape(h, w)
                zw = 16 if (th != 0 and w == 32) else max(0, w - 32)
                zh = 16 if (tv != 0 and h == 32) else max(0, h - 32)
                if zw:
                    c2[:, w - zw:] = 0
                if zh:
                    c2[h - zh:, :] = 0
                b = np.zeros((h, w), np.int16)
                R.ref_xIT(ol.P(ci), w, h, BD, mts, ol.P(b), w)
                rows.append([w, h, mts])
                resi.append(r.reshape(-1))
                coef.append(c)
                back.append(b.reshape(-1))
    z["tr"], z["tr_resi"], z["tr_coef"], z["tr_back"] = np.array(rows, np.int32), np.concatenate(resi), np.concatenate(coef), np.concatenate(back)
    # quant / dequant: w, h, qp, isIRAP, transform skip, absSum; input, levels, dequantised
    rows, cin, lev, deq = [], [], [], []
    for qp in list(range(-24, 64, 8)) + [63]:
        for (w, h, ts) in ((4, 4, 0), (8, 8, 0), (16, 8, 0), (32, 32, 0), (64, 64, 0), (4, 8, 1), (16, 16, 1)):
            if (w == 64 and qp not in (-24, 63)) or (w == 32 and qp % 16):   # the large TUs at a few QPs only: the file stays small
                continue
            if ts:
                c = rng.integers(-4095, 4096, w * h).astype(np.int32)
                c[rng.random(w * h) < 0.25] = 4095
            else:
                c = rng.integers(-32768, 32768, w * h).astype(np.int32)
                c[rng.random(w * h) < 0.4] //= 64
                ext = rng.random(w * h) < 0.25
                c[ext] = np.where(rng.random(int(ext.sum())) < 0.5, -32768, 32767)
                c2 = c.reshape(h, w)
                c2[32:, :] = 0
                c2[:, 32:] = 0
            irap = (qp + w) & 1
            q, d, s = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), C.c_int32()
            R.ref_quant_dequant2(ol.P(c), w, h, BD, qp, irap, ts, ol.P(q), C.byref(s), ol.P(d))
            rows.append([w, h, qp, irap, ts, s.value])
            cin.append(c)
            lev.append(q)
            deq.append(d)
    z["quant"], z["quant_in"], z["quant_lev"], z["quant_deq"] = np.array(rows, np.int32), np.concatenate(cin), np.concatenate(lev), np.concatenate(deq)
    assert z["quant_lev"].max() == 32767 and z["quant_deq"].min() == -32768
    out = os.path.join(HERE, "bd12.npz")
    np.savez_compressed(out, **z)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
