"""Sub-block transform (SBT) for the tests: the reference's rules restated in Python / numpy, the recorded reference results (tests/golden/sbt.npz), the
real reference through ctypes (RefSbt) and job packing plus expectations for the two device entries.

What rests on what.  RefSbt uses only exports the reference library already has: ref_dist (SSE) for partition and tile sums; ref_xT, ref_quant_dequant2 and
ref_xIT with mtsIdx 0 / 2 / 3 / 4 -- exactly the SBT transform pairs (3 = hor DCT-8 / ver DST-7, 4 = hor DST-7 / ver DCT-8) -- for the sub-TU chain; and the
statics CU::getSbtMode, CU::targetSbtAllowed, CU::numSbtModeRdo, CU::getSbtIdxFromSbtMode and CU::getSbtPosFromSbtMode by their mangled names.
PartitionerImpl::getSbtTuTiling (UnitPartitioner.cpp:1091-1148), the SBT branch of TrQuant::getTrTypes (TrQuant.cpp:728-760), CodingUnit::checkAllowedSbt
(Unit.cpp:450-494), the combination step of InterSearch::calcMinDistSbt (InterSearch.cpp:6261-6386) and InterSearch::skipSbtByRDCost (:6389-6438) are members
or take UnitArea / CodingStructure and cannot be called that way: they are RESTATEMENTS here, read against those line ranges."""
import ctypes as C
import os

import numpy as np

import oracle_lib as ol

VER_HALF, HOR_HALF, VER_QUAD, HOR_QUAD = 1, 2, 3, 4
DCT2, DCT8, DST7 = 0, 1, 2
MAX_DIST = (1 << 64) - 1
MAX_DOUBLE = 1.7e+308
U64 = (1 << 64) - 1
MTS_OF = {(DCT2, DCT2): 0, (DST7, DST7): 2, (DCT8, DST7): 3, (DST7, DCT8): 4}   # (trHor, trVer) -> tu.mtsIdx


# ---- section 1: the rules ---------------------------------------------------------------------------------------------------------------------------
def sbt_allowed(w, h, max_tb=64):
    if w > max_tb or h > max_tb:
        return 0
    return (int(w >= 8) << VER_HALF) | (int(h >= 8) << HOR_HALF) | (int(w >= 16) << VER_QUAD) | (int(h >= 16) << HOR_QUAD)


def get_sbt_mode(idx, pos):
    return {VER_HALF: 0, HOR_HALF: 2, VER_QUAD: 4, HOR_QUAD: 6}[idx] + pos


def idx_from_mode(mode):
    return VER_HALF if mode <= 1 else HOR_HALF if mode <= 3 else VER_QUAD if mode <= 5 else HOR_QUAD


def pos_from_mode(mode):
    return mode - get_sbt_mode(idx_from_mode(mode), 0)


def target_allowed(idx, allowed):
    return (allowed >> idx) & 1


def num_mode_rdo(allowed):
    half = target_allowed(VER_HALF, allowed) + target_allowed(HOR_HALF, allowed)
    quad = target_allowed(VER_QUAD, allowed) + target_allowed(HOR_QUAD, allowed)
    return min(2, half << 1) + min(2, quad << 1)


def allowed_modes(w, h):
    a = sbt_allowed(w, h)
    return [m for m in range(8) if target_allowed(idx_from_mode(m), a)]


def coded_tile(cw, ch, idx, pos):
    """(x, y, w, h) of the tile that carries the residual inside a component block cw x ch"""
    size = 1 if idx >= VER_QUAD else 2
    off = 0 if pos == 0 else 4 - size
    if idx in (HOR_HALF, HOR_QUAD):
        return 0, (ch * off) >> 2, cw, (ch * size) >> 2
    return (cw * off) >> 2, 0, (cw * size) >> 2, ch


def tr_types(idx, pos, tw, th):
    """(trHor, trVer) of the luma sub-TU tw x th"""
    if idx in (VER_HALF, VER_QUAD):
        if th > 32:
            return DCT2, DCT2
        return (DCT8, DST7) if pos == 0 else (DST7, DST7)
    if tw > 32:
        return DCT2, DCT2
    return (DST7, DCT8) if pos == 0 else (DST7, DST7)


def dist_shift(bd):
    """DISTORTION_PRECISION_ADJUSTMENT( ( bd - 8 ) << 1 ) of calcMinDistSbt, DISTORTION_PRECISION_ADJUSTMENT( bd ) << 1 of xGetSSE: both 0 in the reference as built (FULL_NBIT = 1, TypeDef.h:228-233) -- distortions keep all bits"""
    return 0


def num_part(side):
    return 4 if side >= 16 else 1 if side == 4 else 2


# ---- section 2: calcMinDistSbt ------------------------------------------------------------------------------------------------------------------------
def part_sums(org, pred, npx, npy, bd):
    """the raw partition sums of one component block: uint32-sized Python ints [4][4]"""
    d = org.astype(np.int64) - pred.astype(np.int64)
    sq = (d * d) >> dist_shift(bd)
    ch, cw = sq.shape
    lx, ly = cw // npx, ch // npy
    out = [[0] * 4 for _ in range(4)]
    for j in range(npy):
        for i in range(npx):
            out[j][i] = int(sq[j * ly:(j + 1) * ly, i * lx:(i + 1) * lx].sum())
    return out


def combine(part, w, h, allowed, chroma_weight, dist_scale):
    """part: [3][4][4] raw sums (absent chroma: zeros) -> dict(est, order, skipAll)"""
    npx, npy = num_part(w), num_part(h)
    dist = [[0] * 4 for _ in range(4)]
    for c in range(3):
        for j in range(npy):
            for i in range(npx):
                s = part[c][j][i]
                dist[j][i] += int(float(s) * chroma_weight) if c else s
    est = [MAX_DIST] * 9
    order = [255] * 8
    est[8] = sum(dist[j][i] for j in range(npy) for i in range(npx))
    if dist_scale * float(est[8]) < float(12 << 15):
        return dict(est=est, order=order, skipAll=1)
    if target_allowed(VER_HALF, allowed):
        resi = sum(dist[j][i] for j in range(npy) for i in range(npx // 2))
        nores = sum(dist[j][i + npx // 2] for j in range(npy) for i in range(npx // 2))
        est[0], est[1] = (resi >> 5) + nores, (nores >> 5) + resi
    if target_allowed(HOR_HALF, allowed):
        resi = sum(dist[j][i] for j in range(npy // 2) for i in range(npx))
        nores = sum(dist[j + npy // 2][i] for j in range(npy // 2) for i in range(npx))
        est[2], est[3] = (resi >> 5) + nores, (nores >> 5) + resi
    if target_allowed(VER_QUAD, allowed):
        est[4] = sum(dist[j][0] + ((dist[j][1] + dist[j][2] + dist[j][3]) << 5) for j in range(npy)) >> 5
        est[5] = sum(dist[j][3] + ((dist[j][0] + dist[j][1] + dist[j][2]) << 5) for j in range(npy)) >> 5
    if target_allowed(HOR_QUAD, allowed):
        est[6] = sum(dist[0][i] + ((dist[1][i] + dist[2][i] + dist[3][i]) << 5) for i in range(npx)) >> 5
        est[7] = sum(dist[3][i] + ((dist[0][i] + dist[1][i] + dist[2][i]) << 5) for i in range(npx)) >> 5
    temp, pos = list(est[:8]), 0
    for first, types in ((0, (VER_HALF, HOR_HALF)), (4, (VER_QUAD, HOR_QUAD))):
        num = min(sum(target_allowed(t, allowed) for t in types) << 1, 2)
        for _ in range(num):
            best, min_dist = 255, MAX_DIST
            for m in range(first, first + 4):
                if temp[m] < min_dist:
                    min_dist, best = temp[m], m
            order[pos] = best
            temp[best] = MAX_DIST
            pos += 1
    return dict(est=est, order=order, skipAll=0)


def skip_by_rdcost(est, dist_scale, idx, pos, best_cost, dist_sbt_off, cost_sbt_off, root_cbf_sbt_off):
    mode = get_sbt_mode(idx, pos)
    if dist_scale * float(est[mode]) + float(11 << 15) > best_cost:
        return 0
    if cost_sbt_off != MAX_DOUBLE:
        if not root_cbf_sbt_off:
            diff = (est[8] - est[mode]) & U64
            resi_part = ((diff * 9) & U64) >> 4 if idx in (VER_HALF, HOR_HALF) else ((diff * 3) & U64) >> 3
            est_cost = (cost_sbt_off - (dist_scale * float(dist_sbt_off) + 0.0)) + (dist_scale * float((est[mode] + resi_part) & U64) + float(10 << 15))
            if est_cost > cost_sbt_off:
                return 1
            if est_cost > best_cost:
                return 2
        else:
            weight = 0.4 if mode > 3 else 0.6
            est_cost = ((cost_sbt_off - (dist_scale * float(dist_sbt_off) + 0.0)) * weight) + (dist_scale * float(est[mode]) + 0.0)
            if est_cost > best_cost:
                return 3
    return 255


# ---- section 3: one component of a candidate ----------------------------------------------------------------------------------------------------------
def chain_expect(r, idx, pos, luma, bd, qp_per, qp_rem, irap):
    """r: the CU's residual block of one component (ch x cw).  The sub-TU through the oracle's xT -> quant -> dequant -> xIT with the SBT transform pair, the
    CU-shaped reconstruction and the two SSEs."""
    L = ol.oracle()
    ch, cw = r.shape
    x, y, w, h = coded_tile(cw, ch, idx, pos)
    th, tv = tr_types(idx, pos, w, h) if luma else (DCT2, DCT2)
    sub = np.ascontiguousarray(r[y:y + h, x:x + w], np.int16)
    coef, qc, dq = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
    s = C.c_int32()
    rec_sub = np.zeros((h, w), np.int16)
    assert L.vo_fwd_2d(ol.P(sub), w, w, h, bd, th, tv, ol.P(coef)) == 0
    L.vo_quant(ol.P(coef), w, h, bd, qp_per, qp_rem, irap, 0, ol.P(qc), None, C.byref(s))
    L.vo_dequant(ol.P(qc), w, h, bd, qp_per, qp_rem, 0, ol.P(dq))
    assert L.vo_inv_2d(ol.P(dq), w, h, bd, th, tv, ol.P(rec_sub), w) == 0
    return finish_expect(r, (x, y, w, h), (th, tv), qc, rec_sub, s.value, bd)


def finish_expect(r, tile, types, levels, rec_sub, abs_sum, bd):
    x, y, w, h = tile
    rec = np.zeros(r.shape, np.int16)
    rec[y:y + h, x:x + w] = rec_sub
    d = r[y:y + h, x:x + w].astype(np.int64) - rec_sub
    zero = (r.astype(np.int64) ** 2) >> dist_shift(bd)
    zero[y:y + h, x:x + w] = 0
    return dict(tile=tile, types=types, levels=np.asarray(levels, np.int32).reshape(-1), rec_sub=rec_sub, rec=rec, sseCoded=int((d * d).sum()), sseZero=int(zero.sum()),
                absSum=int(abs_sum))


# ---- the recorded reference results ----------------------------------------------------------------------------------------------------------------------
GOLDEN_SHAPES = [(4, 8), (8, 4), (8, 8), (16, 8), (8, 16), (16, 16), (64, 16), (16, 64), (32, 32), (64, 32), (32, 64), (64, 64)]   # (cuW, cuH), luma


def golden_case_inputs():
    """(cuW, cuH, mode, luma, bd, qp, irap, residual block of the component): every shape and allowed mode on the luma block, and on the 4:2:0 chroma block of the
    CU; bit depth, QP and slice type rotate; every fourth case has a residual small enough to quantise to zero"""
    rng = np.random.default_rng(20261)
    k = 0
    for (w, h) in GOLDEN_SHAPES:
        for mode in allowed_modes(w, h):
            for luma in (1, 0):
                bd, qp, irap = (8, 10, 12)[k % 3], (22, 32, 42)[(k // 3) % 3], (k // 2) % 2
                amp = 1 if k % 4 == 3 else min((1 << bd) - 1, 40 << (bd - 8))
                cw, ch = (w, h) if luma else (w // 2, h // 2)
                yield w, h, mode, luma, bd, qp, irap, rng.integers(-amp, amp + 1, (ch, cw)).astype(np.int16)
                k += 1


def golden():
    z = np.load(os.path.join(ol.ROOT, "tests", "golden", "sbt.npz"))
    return {k: z[k] for k in z.files}


def golden_cases(z=None):
    """yields dict(w, h, mode, luma, bd, qp, irap, resi, levels, rec_sub, sse, absSum, part) per recorded case"""
    z = z or golden()
    for k in range(len(z["w"])):
        w, h, mode, luma = int(z["w"][k]), int(z["h"][k]), int(z["mode"][k]), int(z["luma"][k])
        cw, ch = (w, h) if luma else (w // 2, h // 2)
        _, _, tw, th = coded_tile(cw, ch, idx_from_mode(mode), pos_from_mode(mode))
        o, so = int(z["off"][k]), int(z["sub_off"][k])
        yield dict(w=w, h=h, mode=mode, luma=luma, bd=int(z["bd"][k]), qp=int(z["qp"][k]), irap=int(z["irap"][k]), resi=z["resi"][o:o + cw * ch].reshape(ch, cw),
                   levels=z["levels"][so:so + tw * th], rec_sub=z["rec"][so:so + tw * th].reshape(th, tw), sse=int(z["sse"][k]), absSum=int(z["abs_sum"][k]),
                   part=z["part"][k].tolist())


def qp_of(qp, bd):
    """QpParam::per / rem of a base QP at this bit depth (Quant.cpp:65-104)"""
    return divmod(qp + 6 * (bd - 8), 6)


# ---- the real reference (oracle/_ref/libvtmref.so) --------------------------------------------------------------------------------------------------------
class RefSbt:
    def __init__(self, L):
        self.L = L
        u8 = C.c_uint8
        for name, sym, nargs in (("get_sbt_mode", "_ZN2CU10getSbtModeEhh", 2), ("target_allowed", "_ZN2CU16targetSbtAllowedEhh", 2), ("num_mode_rdo", "_ZN2CU13numSbtModeRdoEh", 1),
                                 ("idx_from_mode", "_ZN2CU20getSbtIdxFromSbtModeEh", 1), ("pos_from_mode", "_ZN2CU20getSbtPosFromSbtModeEh", 1)):
            fn = getattr(L, sym)
            fn.restype, fn.argtypes = u8, [u8] * nargs
            setattr(self, name, fn)

    def sse(self, a, b, bd):
        """RdCost::xGetSSE over two blocks of one shape (any strides)"""
        h, w = a.shape
        assert a.strides[1] == 2 and b.strides[1] == 2
        return int(self.L.ref_dist(2, 0, C.c_void_p(a.ctypes.data), a.strides[0] // 2, C.c_void_p(b.ctypes.data), b.strides[0] // 2, w, h, bd, 0))

    def part_sums(self, org, pred, npx, npy, bd):
        ch, cw = org.shape
        lx, ly = cw // npx, ch // npy
        out = [[0] * 4 for _ in range(4)]
        for j in range(npy):
            for i in range(npx):
                out[j][i] = self.sse(org[j * ly:(j + 1) * ly, i * lx:(i + 1) * lx], pred[j * ly:(j + 1) * ly, i * lx:(i + 1) * lx], bd)
        return out

    def chain(self, r, idx, pos, luma, bd, qp, irap):
        """the sub-TU through the real TrQuant::xT, Quant::quant / dequant and TrQuant::xIT; the tile SSEs through the real xGetSSE"""
        ch, cw = r.shape
        x, y, w, h = coded_tile(cw, ch, idx, pos)
        types = tr_types(idx, pos, w, h) if luma else (DCT2, DCT2)
        mts = MTS_OF[types]
        sub = np.ascontiguousarray(r[y:y + h, x:x + w], np.int16)
        coef, qc, dq = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
        s = C.c_int32()
        rec_sub = np.zeros((h, w), np.int16)
        self.L.ref_xT(ol.P(sub), w, w, h, bd, mts, ol.P(coef))
        self.L.ref_quant_dequant2(ol.P(coef), w, h, bd, qp, irap, mts, ol.P(qc), C.byref(s), ol.P(dq))
        self.L.ref_xIT(ol.P(dq), w, h, bd, mts, ol.P(rec_sub), w)
        e = finish_expect(r, (x, y, w, h), types, qc, rec_sub, s.value, bd)
        assert e["sseCoded"] == self.sse(sub, rec_sub, bd)
        if idx < VER_QUAD:   # a half mode's uncoded tile is the other position's coded tile: its SSE against zero through the real member
            zx, zy, zw, zh = coded_tile(cw, ch, idx, 1 - pos)
            blk = np.ascontiguousarray(r[zy:zy + zh, zx:zx + zw])
            assert e["sseZero"] == self.sse(blk, np.zeros_like(blk), bd)
        return e


# ---- device batches ------------------------------------------------------------------------------------------------------------------------------------
def comp_shape(w, h, c):
    return (w, h) if c == 0 else (w // 2, h // 2)


class EstBatch:
    """Estimator jobs on strided planes with random samples around the blocks.  specs: list of dict(w, h, bd, chroma (bool), allowed, cw (chroma weight), ds
    (distScale), blocks=[(org, pred)] * (3 or 1))."""

    def __init__(self, specs, seed=1):
        from vtm_amd.lib import SbtEstJob
        rng = np.random.default_rng(seed)
        n = len(specs)
        self.n, self.specs = n, specs
        self.stride = 200
        rows = 66
        self.org = rng.integers(0, 256, (n * rows, self.stride)).astype(np.int16)
        self.pred = rng.integers(0, 256, (n * rows, self.stride)).astype(np.int16)
        self.jobs = (SbtEstJob * n)()
        self.exp = []
        cols = (3, 71, 110)   # Y, Cb, Cr side by side in the job's band of rows; odd luma column: unaligned pairs
        for k, s in enumerate(specs):
            j = self.jobs[k]
            j.width, j.height, j.bitDepth, j.sbtAllowed, j.chromaWeight, j.distScale = s["w"], s["h"], s["bd"], s["allowed"], s["cw"], s["ds"]
            part = [[[0] * 4 for _ in range(4)] for _ in range(3)]
            for c in range(3):
                if c and not s["chroma"]:
                    j.orgOff[c] = j.predOff[c] = -1
                    continue
                o, p = s["blocks"][c]
                ch, cw = o.shape
                r0 = k * rows + 1
                self.org[r0:r0 + ch, cols[c]:cols[c] + cw] = o
                self.pred[r0:r0 + ch, cols[c]:cols[c] + cw] = p
                j.orgOff[c] = j.predOff[c] = r0 * self.stride + cols[c]
                j.orgStride[c] = j.predStride[c] = self.stride
                part[c] = part_sums(o, p, num_part(s["w"]), num_part(s["h"]), s["bd"])
            e = combine(part, s["w"], s["h"], s["allowed"], s["cw"], s["ds"])
            e["part"] = part
            self.exp.append(e)

    def run(self, ctx, idx=None):
        from vtm_amd.lib import SbtEstJob, SbtEstResult
        idx = list(range(self.n)) if idx is None else idx
        sub = (SbtEstJob * len(idx))()
        for i, k in enumerate(idx):
            C.memmove(C.byref(sub[i]), C.byref(self.jobs[k]), C.sizeof(SbtEstJob))
        d_org, d_pred, d_jobs = ctx.to_device(self.org), ctx.to_device(self.pred), ctx.to_device(np.frombuffer(sub, np.uint8))
        d_res = ctx.to_device(np.full(C.sizeof(SbtEstResult) * len(idx), 0xA5, np.uint8))
        ctx.sbt_est_batch(d_org.ptr, d_pred.ptr, d_jobs.ptr, len(idx), max(self.specs[k]["w"] for k in idx), max(self.specs[k]["h"] for k in idx), d_res.ptr)
        res = (SbtEstResult * len(idx)).from_buffer_copy(d_res.to_host(np.uint8).tobytes())
        for d in (d_org, d_pred, d_jobs, d_res):
            d.free()
        return res

    def check(self, res, idx=None):
        idx = list(range(self.n)) if idx is None else idx
        for i, k in enumerate(idx):
            e, r, s = self.exp[k], res[i], self.specs[k]
            tag = (k, s["w"], s["h"], s["bd"], s["chroma"], s["allowed"])
            assert [[list(r.part[c][j]) for j in range(4)] for c in range(3)] == e["part"], ("part", tag)
            assert list(r.est) == e["est"], ("est", tag, list(r.est), e["est"])
            assert list(r.rdoOrder) == e["order"] and r.skipAll == e["skipAll"], ("order / skipAll", tag, list(r.rdoOrder), e["order"], r.skipAll)
            assert list(r.pad) == [0] * 7


def est_spec(rng, w, h, bd, chroma, amp, cw=0.8137, ds=None, allowed=None):
    """a random CU: samples over the full range of the bit depth, |org - pred| <= amp"""
    top = (1 << bd) - 1
    blocks = []
    for c in range(3 if chroma else 1):
        bw, bh = comp_shape(w, h, c)
        o = rng.integers(0, top + 1, (bh, bw)).astype(np.int64)
        p = np.clip(o + rng.integers(-amp, amp + 1, (bh, bw)), 0, top)
        blocks.append((o.astype(np.int16), p.astype(np.int16)))
    return dict(w=w, h=h, bd=bd, chroma=chroma, allowed=sbt_allowed(w, h) if allowed is None else allowed, cw=cw, ds=1.0 / 57.3 if ds is None else ds, blocks=blocks)


class ChainBatch:
    """Chain candidates on a strided residual plane with random samples around the blocks.  specs: list of dict(w, h, mode, bd, qp, irap, chroma (bool),
    resi=[block] * (3 or 1)).  Output slots: comp c of candidate k at (3 k + c) * slot."""

    SLOT = 4096 + 64

    def __init__(self, specs, seed=2):
        from vtm_amd.lib import SbtJob
        rng = np.random.default_rng(seed)
        n = len(specs)
        self.n, self.specs, self.stride = n, specs, 200
        rows = 66
        self.resi = rng.integers(-300, 301, (n * rows, self.stride)).astype(np.int16)
        self.jobs = (SbtJob * n)()
        self.exp = []
        cols = (3, 71, 110)
        for k, s in enumerate(specs):
            j = self.jobs[k]
            idx, pos = idx_from_mode(s["mode"]), pos_from_mode(s["mode"])
            j.width, j.height, j.sbtIdx, j.sbtPos, j.bitDepth, j.isIRAP = s["w"], s["h"], idx, pos, s["bd"], s["irap"]
            es = []
            for c in range(3):
                if c and not s["chroma"]:
                    j.resiOff[c] = -1
                    es.append(None)
                    continue
                r = s["resi"][c]
                ch, cw = r.shape
                r0 = k * rows + 1
                self.resi[r0:r0 + ch, cols[c]:cols[c] + cw] = r
                per, rem = qp_of(s["qp"] if c == 0 else s.get("qpc", s["qp"] + 1), s["bd"])   # chroma with a QP of its own
                j.resiOff[c], j.resiStride[c], j.outOff[c], j.qpPer[c], j.qpRem[c] = r0 * self.stride + cols[c], self.stride, (3 * k + c) * self.SLOT + 7, per, rem
                es.append(chain_expect(r, idx, pos, c == 0, s["bd"], per, rem, s["irap"]))
            self.exp.append(es)

    def sub_jobs(self, idx=None):
        from vtm_amd.lib import SbtJob
        idx = list(range(self.n)) if idx is None else idx
        sub = (SbtJob * len(idx))()
        for i, k in enumerate(idx):
            C.memmove(C.byref(sub[i]), C.byref(self.jobs[k]), C.sizeof(SbtJob))
        return sub

    def run(self, ctx, idx=None, levels=True, rec=True):
        from vtm_amd.lib import SbtResult
        idx = list(range(self.n)) if idx is None else idx
        sub = self.sub_jobs(idx)
        d_resi, d_jobs = ctx.to_device(self.resi), ctx.to_device(np.frombuffer(sub, np.uint8))
        d_res = ctx.to_device(np.full(C.sizeof(SbtResult) * len(idx), 0xA5, np.uint8))
        d_lv, d_rec = ctx.to_device(np.full((3 * self.n, self.SLOT), -7, np.int32)), ctx.to_device(np.full((3 * self.n, self.SLOT), -7, np.int16))
        ctx.sbt_chain_batch(d_resi.ptr, d_jobs.ptr, len(idx), d_res.ptr, d_lv.ptr if levels else None, d_rec.ptr if rec else None)
        res = (SbtResult * len(idx)).from_buffer_copy(d_res.to_host(np.uint8).tobytes())
        out = res, d_lv.to_host().reshape(3 * self.n, self.SLOT), d_rec.to_host().reshape(3 * self.n, self.SLOT)
        for d in (d_resi, d_jobs, d_res, d_lv, d_rec):
            d.free()
        return out

    def check(self, got, idx=None, levels=True, rec=True):
        res, lv, rc = got
        idx = list(range(self.n)) if idx is None else idx
        touched = set()
        for i, k in enumerate(idx):
            s, r = self.specs[k], res[i]
            for c in range(3):
                e, tag = self.exp[k][c], (k, c, s["w"], s["h"], s["mode"], s["bd"], s["qp"])
                g = (r.sseCoded[c], r.sseZero[c], r.absSum[c])
                if e is None:
                    assert g == (0, 0, 0), tag
                    continue
                assert g == (e["sseCoded"], e["sseZero"], e["absSum"]), (tag, g, (e["sseCoded"], e["sseZero"], e["absSum"]))
                row, (cw, ch), (_, _, tw, th) = 3 * k + c, comp_shape(s["w"], s["h"], c), e["tile"]
                touched.add(row)
                if levels:
                    assert np.array_equal(lv[row, 7:7 + tw * th], e["levels"]), ("levels", tag)
                    assert (lv[row, :7] == -7).all() and (lv[row, 7 + tw * th:] == -7).all(), ("levels outside the block", tag)
                if rec:
                    assert np.array_equal(rc[row, 7:7 + cw * ch].reshape(ch, cw), e["rec"]), ("rec", tag)
                    assert (rc[row, :7] == -7).all() and (rc[row, 7 + cw * ch:] == -7).all(), ("rec outside the block", tag)
            assert r.pad == 0
        for row in range(3 * self.n):
            if row not in touched or not levels:
                assert (lv[row] == -7).all()
            if row not in touched or not rec:
                assert (rc[row] == -7).all()

    def assert_bites(self):
        """on the EXPECTED values: at least half of the coded luma sub-TUs have levels, and some have none"""
        luma = [es[0]["absSum"] for es in self.exp]
        assert sum(a > 0 for a in luma) * 2 >= len(luma) and any(a == 0 for a in luma), (sum(a > 0 for a in luma), len(luma))


def chain_spec(rng, w, h, mode, bd, qp, irap, chroma, amp):
    top = (1 << bd) - 1
    amp = min(amp, top)
    return dict(w=w, h=h, mode=mode, bd=bd, qp=qp, irap=irap, chroma=chroma,
                resi=[rng.integers(-amp, amp + 1, comp_shape(w, h, c)[::-1]).astype(np.int16) for c in range(3 if chroma else 1)])
