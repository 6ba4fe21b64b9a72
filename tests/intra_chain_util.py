"""Tables, buffers and expectations of the intra residual chain (vtmhip_intra_chain_batch_dev) for the CPU and GPU tests.

A Level is a list of intra_util.make_block dicts -- `modes`: the regular modes, `mip`: (mode, transposed) pairs, both may be empty -- placed in an original plane
(intra_util.place_in_plane), and a list of TU specs (pred, typeHor, typeVer, qp, irap).  Predictions are numbered as the entry numbers them: the regular jobs block
after block, then the MIP jobs.  Every prediction / output block lies between GAP samples of fill, at offsets that are only 2-byte aligned."""
import ctypes as C

import numpy as np

import intra_util as iu
import mip_util as mu
import oracle_lib as ol
from vtm_amd import lib
from vtm_amd.lib import IntraBlock, IntraJob, IntraTuJob, IntraTuResult, MipJob, TuJob, TuResult

GAP = 5
FILL = 0xa5
FILL16 = np.frombuffer(bytes([FILL, FILL]), np.int16)[0]
FILL32 = np.frombuffer(bytes([FILL] * 4), np.int32)[0]
TU_FIELDS = [f for f, _ in TuJob._fields_]


def qp_of(qp, bd, ts=False):
    """QpParam::per / rem of a base QP at this bit depth (Quant.cpp:65-104); transform skip: the floor of 4 on the base QP"""
    base = qp + 6 * (bd - 8)
    return divmod(max(base, 4) if ts else base, 6)


def expand(blocks, intra_jobs, n_intra, mip_jobs, tu_jobs):
    """the Python restatement of vtmhip_intra_chain_make_tu_jobs over ctypes arrays: ([dict of every vtmhip_tu_job field], maxWidth, maxHeight, uniform)"""
    out, sizes, ts = [], set(), False
    for t in tu_jobs:
        j = intra_jobs[t.pred] if t.pred < n_intra else mip_jobs[t.pred - n_intra]
        b = blocks[j.block]
        out.append(dict(resiOff=j.predOff, outOff=t.outOff, resiStride=b.width, width=b.width, height=b.height, qpPer=t.qpPer, qpRem=t.qpRem, typeHor=t.typeHor,
                        typeVer=t.typeVer, bitDepth=b.bitDepth, isIRAP=t.isIRAP, pad=0, chromaAdj=0))
        sizes.add((b.width, b.height))
        ts |= t.typeHor == lib.TRSKIP
    mw, mh = max([w for w, _ in sizes] + [0]), max([h for _, h in sizes] + [0])
    return out, mw, mh, int(len(sizes) == 1 and not ts)


def tu_fields(j):
    return {f: getattr(j, f) for f in TU_FIELDS}


class Level:
    def __init__(self, blocks, plane, tus, order=None):
        self.blocks, self.plane = blocks, plane
        self.ref_buf, ref_offs = iu.embed([(b["top"], b["left"]) for b in blocks])
        self.blk_arr = (IntraBlock * max(len(blocks), 1))()
        ij, mj, off = [], [], GAP
        for i, b in enumerate(blocks):
            self.blk_arr[i] = IntraBlock(ref_offs[i], b["org_off"], b["org_stride"], b["w"], b["h"], b["bd"], b["m"])
        for i, b in enumerate(blocks):
            for mode in b["modes"]:
                ij.append((i, mode, off))
                off += b["w"] * b["h"] + GAP
        for i, b in enumerate(blocks):
            for mode, t in b.get("mip", []):
                mj.append((i, mode, t, off))
                off += b["w"] * b["h"] + GAP
        self.pred_len = off
        self.preds = [(i, o) for i, _, o in ij] + [(i, o) for i, _, _, o in mj]      # prediction p -> (block, predOff)
        self.n_intra, self.n_mip = len(ij), len(mj)
        self.intra_arr = (IntraJob * max(len(ij), 1))(*[IntraJob(o, i, mode) for i, mode, o in ij])
        self.mip_arr = (MipJob * max(len(mj), 1))(*[MipJob(o, i, mode, t) for i, mode, t, o in mj])
        self.ij, self.mj = ij, mj
        tus = [tus[k] for k in order] if order is not None else list(tus)
        self.tus, off, arr = tus, GAP, []
        for p, th, tv, qp, irap in tus:
            b = blocks[self.preds[p][0]]
            per, rem = qp_of(qp, b["bd"], th == lib.TRSKIP)
            arr.append(IntraTuJob(off, p, per, rem, th, tv, irap, 0, 0))
            off += b["w"] * b["h"] + GAP
        self.out_len, self.n_tu = off, len(tus)
        self.tu_arr = (IntraTuJob * max(len(tus), 1))(*arr)
        self._exp = None

    def block_of_tu(self, k):
        return self.blocks[self.preds[self.tu_arr[k].pred][0]]

    def org_of(self, b):
        x, y = b["org_xy"]
        return self.plane[y:y + b["h"], x:x + b["w"]].astype(np.int64)

    def tu_jobs(self):
        jobs, mw, mh, uni = expand(self.blk_arr, self.intra_arr, self.n_intra, self.mip_arr, [self.tu_arr[k] for k in range(self.n_tu)])
        return (TuJob * max(self.n_tu, 1))(*[TuJob(*[j[f] for f in TU_FIELDS]) for j in jobs]), mw, mh, uni

    def device_args(self, ctx, levels=True, n_tu=None, n_intra=None, n_mip=None):
        """the tables uploaded and the five output buffers pre-filled with FILL: (the arguments of Context.intra_chain_batch in order, inputs, outputs)"""
        from vtm_amd.device import struct_array_to_numpy as s2n
        n_tu = self.n_tu if n_tu is None else n_tu
        n_intra = self.n_intra if n_intra is None else n_intra
        n_mip = self.n_mip if n_mip is None else n_mip
        ins = [ctx.to_device(a) for a in (self.ref_buf, self.plane, s2n(self.blk_arr), s2n(self.intra_arr), s2n(self.mip_arr), s2n(self.tu_arr))]
        outs = [ctx.to_device(np.full(n, FILL, np.uint8)) for n in (2 * self.pred_len, 2 * self.pred_len, 4 * self.out_len, 2 * self.out_len, 24 * max(self.n_tu, 1))]
        args = [ins[0].ptr, ins[1].ptr, ins[2].ptr, len(self.blocks), ins[3].ptr, n_intra, ins[4].ptr, n_mip, ins[5].ptr, n_tu, outs[0].ptr, outs[1].ptr, outs[3].ptr,
                outs[4].ptr, outs[2].ptr if levels else None]
        return args, ins, outs

    # ---- the device call ----------------------------------------------------------------------------------------------------------------------------------
    def run(self, ctx, levels=True, n_tu=None, n_intra=None, n_mip=None):
        """-> dict of the five output buffers as numpy arrays (levels None when not asked for), every one pre-filled with FILL"""
        args, ins, outs = self.device_args(ctx, levels, n_tu, n_intra, n_mip)
        status = lib.OK
        try:
            ctx.intra_chain_batch(*args)
        except lib.VtmHipError as e:
            status = e.status
        ctx.sync()
        got = dict(status=status, pred=outs[0].to_host(np.int16, shape=(-1,)), resi=outs[1].to_host(np.int16, shape=(-1,)), levels=outs[2].to_host(np.int32, shape=(-1,)), reco=outs[3].to_host(np.int16, shape=(-1,)),
                   results=np.frombuffer(outs[4].to_host(np.uint8, shape=(-1,)).tobytes(), np.dtype([("sse", "<u8"), ("sseResi", "<u8"), ("sumAbs", "<i4"), ("absSum", "<i4")])))
        for b in ins + outs:
            b.free()
        return got

    # ---- the composed expectation: entries that are pinned to the reference, numpy between them ---------------------------------------------------------------------
    def expect(self, ctx):
        if self._exp is not None:
            return self._exp
        from vtm_amd.device import struct_array_to_numpy as s2n
        d_ref, d_blk = ctx.to_device(self.ref_buf), ctx.to_device(s2n(self.blk_arr))
        d_pred = ctx.to_device(np.full(2 * self.pred_len, FILL, np.uint8))
        d_ij, d_mj = ctx.to_device(s2n(self.intra_arr)), ctx.to_device(s2n(self.mip_arr))
        if self.n_intra:
            ctx.intra_pred_batch(d_ref.ptr, d_blk.ptr, len(self.blocks), d_ij.ptr, self.n_intra, d_pred.ptr)
        if self.n_mip:
            ctx.mip_pred_batch(d_ref.ptr, d_blk.ptr, len(self.blocks), d_mj.ptr, self.n_mip, d_pred.ptr)
        ctx.sync()
        pred = d_pred.to_host(np.int16, shape=(-1,))
        resi = np.full(self.pred_len, FILL16, np.int16)
        for i, off in self.preds:
            b = self.blocks[i]
            n = b["w"] * b["h"]
            resi[off:off + n] = (self.org_of(b).reshape(-1) - pred[off:off + n]).astype(np.int16)
        levels, reco = np.full(self.out_len, FILL32, np.int32), np.full(self.out_len, FILL16, np.int16)
        results, clipped = [], [0, 0]
        bufs = [d_ref, d_blk, d_pred, d_ij, d_mj]
        if self.n_tu:
            jobs, mw, mh, _ = self.tu_jobs()
            d_resi, d_jobs = ctx.to_device(resi), ctx.to_device(s2n(jobs))
            d_lev, d_rec, d_res = ctx.to_device(levels), ctx.to_device(reco), ctx.alloc(16 * self.n_tu)
            ctx.tu_chain_batch(d_resi.ptr, d_jobs.ptr, self.n_tu, mw, mh, d_res.ptr, d_lev.ptr, d_rec.ptr, uniform=False)
            ctx.sync()
            levels, reco = d_lev.to_host(np.int32, shape=(-1,)), d_rec.to_host(np.int16, shape=(-1,)).copy()
            tres = (TuResult * self.n_tu).from_buffer_copy(d_res.to_host(np.uint8, shape=(-1,)).tobytes())
            bufs += [d_resi, d_jobs, d_lev, d_rec, d_res]
            for k in range(self.n_tu):
                t, b = self.tu_arr[k], self.block_of_tu(k)
                n, po = b["w"] * b["h"], self.preds[t.pred][1]
                raw = pred[po:po + n].astype(np.int64) + reco[t.outOff:t.outOff + n]
                rec = np.clip(raw, 0, (1 << b["bd"]) - 1)
                clipped[0] += int((raw < 0).sum())
                clipped[1] += int((raw > (1 << b["bd"]) - 1).sum())
                reco[t.outOff:t.outOff + n] = rec
                d = self.org_of(b).reshape(-1) - rec
                results.append((int((d * d).sum()), int(tres[k].sse), int(tres[k].sumAbs), int(tres[k].absSum)))
        for b in bufs:
            b.free()
        self._exp = dict(pred=pred, resi=resi, levels=levels, reco=reco, results=results, clipped=clipped)
        return self._exp

    def check(self, got, exp, levels=True):
        """every buffer in full: the blocks and the fill between them"""
        assert np.array_equal(got["pred"], exp["pred"]), np.argwhere(got["pred"] != exp["pred"])[:6].tolist()
        assert np.array_equal(got["resi"], exp["resi"]), np.argwhere(got["resi"] != exp["resi"])[:6].tolist()
        if levels:
            assert np.array_equal(got["levels"], exp["levels"]), np.argwhere(got["levels"] != exp["levels"])[:6].tolist()
        else:
            assert (got["levels"] == FILL32).all()
        assert np.array_equal(got["reco"], exp["reco"]), np.argwhere(got["reco"] != exp["reco"])[:6].tolist()
        res = [tuple(int(v) for v in r) for r in got["results"][:self.n_tu]]
        assert res == exp["results"], [(k, a, b) for k, (a, b) in enumerate(zip(res, exp["results"])) if a != b][:4]

    def untouched(self, got):
        return all((got[k].view(np.uint8) == FILL).all() for k in ("pred", "resi", "levels", "reco")) and (got["results"].view(np.uint8) == FILL).all()

    # ---- without any device entry: the restatements and the oracle ------------------------------------------------------------------------------------------------
    def oracle_expect(self, k):
        """TU job k from intra_util / mip_util and the oracle's xT -> quant -> dequant -> xIT: dict(pred, resi, levels, reco, result)"""
        L = ol.oracle()
        t, b = self.tu_arr[k], self.block_of_tu(k)
        w, h, bd = b["w"], b["h"], b["bd"]
        if t.pred < self.n_intra:
            pred = iu.predict(b["top"], b["left"], w, h, self.ij[t.pred][1], b["m"], bd, [])
        else:
            _, mode, tr, _ = self.mj[t.pred - self.n_intra]
            pred = mu.predict(b["top"], b["left"], w, h, mode, tr, bd)
        org = self.org_of(b)
        resi = np.ascontiguousarray(org - pred, np.int16)
        coef, qc, dq = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
        s, rec = C.c_int32(), np.zeros((h, w), np.int16)
        ts = int(t.typeHor == lib.TRSKIP)
        if ts:
            coef[:] = resi.reshape(-1)
        else:
            assert L.vo_fwd_2d(ol.P(resi), w, w, h, bd, t.typeHor, t.typeVer, ol.P(coef)) == 0
        L.vo_quant(ol.P(coef), w, h, bd, t.qpPer, t.qpRem, t.isIRAP, ts, ol.P(qc), None, C.byref(s))
        L.vo_dequant(ol.P(qc), w, h, bd, t.qpPer, t.qpRem, ts, ol.P(dq))
        if ts:
            rec[:] = dq.reshape(h, w).astype(np.int16)       # xITransformSkip: Pel( coefficient )
        else:
            assert L.vo_inv_2d(ol.P(dq), w, h, bd, t.typeHor, t.typeVer, ol.P(rec), w) == 0
        raw = pred.astype(np.int64) + rec
        reco = np.clip(raw, 0, (1 << bd) - 1)
        d, dr = org - reco, resi.astype(np.int64) - rec
        return dict(pred=pred.reshape(-1), resi=resi.reshape(-1), levels=qc, reco=reco.reshape(-1).astype(np.int16), raw=raw,
                    result=(int((d * d).sum()), int((dr * dr).sum()), int(np.abs(coef.astype(np.int64)).sum()), s.value))

    def check_oracle(self, got, k):
        t, b = self.tu_arr[k], self.block_of_tu(k)
        n, po, e = b["w"] * b["h"], self.preds[t.pred][1], self.oracle_expect(k)
        assert np.array_equal(got["pred"][po:po + n], e["pred"]) and np.array_equal(got["resi"][po:po + n], e["resi"]), k
        assert np.array_equal(got["levels"][t.outOff:t.outOff + n], e["levels"]) and np.array_equal(got["reco"][t.outOff:t.outOff + n], e["reco"]), k
        assert tuple(int(v) for v in got["results"][k]) == e["result"], (k, got["results"][k], e["result"])


def make_level(rng, shapes, tus_of, kind="random", stride=97, order=None):
    """shapes: (w, h, m, bd, modes, mip[, kind]) per block; tus_of( p, block dict ) -> the (typeHor, typeVer, qp, irap) candidates of prediction p.
    A block of kind 'const' has constant lines, so every prediction is that constant; its original is the constant +- 1: a residual that quantises to nothing"""
    blocks = []
    for spec in shapes:
        w, h, m, bd, modes, mip = spec[:6]
        b = iu.make_block(rng, w, h, m, bd, spec[6] if len(spec) > 6 else kind, modes)
        b["mip"], b["kind"] = list(mip), spec[6] if len(spec) > 6 else kind
        blocks.append(b)
    plane = iu.place_in_plane(rng, blocks, stride)
    for b in blocks:
        if b["kind"] == "const":
            (x, y), v = b["org_xy"], int(b["top"][1])
            plane[y:y + b["h"], x:x + b["w"]] = np.clip(v + rng.integers(-1, 2, (b["h"], b["w"])), 0, (1 << b["bd"]) - 1)
    preds = [i for i, b in enumerate(blocks) for _ in b["modes"]] + [i for i, b in enumerate(blocks) for _ in b["mip"]]
    tus = [(p, th, tv, qp, irap) for p, i in enumerate(preds) for th, tv, qp, irap in tus_of(p, blocks[i])]
    return Level(blocks, plane, tus, order)


# ---- malformed tables: one defect each, applied to a fresh base_level ---------------------------------------------------------------------------------------------
def base_level(seed=5):
    """three blocks (8x8 on line 0, 16x4 on line 1, 64x16 on line 0), regular and MIP jobs on them, one or two candidates per prediction"""
    shapes = [(8, 8, 0, 10, [0, 1, 50], [(0, 0), (7, 1)]), (16, 4, 1, 8, [1, 18], []), (64, 16, 0, 12, [34], [(5, 1)])]
    return make_level(np.random.default_rng(seed), shapes, lambda p, b: [(lib.DCT2, lib.DCT2, 30, p & 1)] + ([(lib.DST7, lib.DCT8, 27, 0)] if b["w"] <= 32 and p % 3 == 0 else []))


def _set(table, k, field, v, idx=None):
    def f(lv):
        rec = getattr(lv, table)[k]
        if idx is None:
            setattr(rec, field, v)
        else:
            getattr(rec, field)[idx] = v
    return f


def _tu_of_block(lv, blk):
    return next(k for k in range(lv.n_tu) if lv.preds[lv.tu_arr[k].pred][0] == blk)


def _set_tu_of_block(blk, **fields):
    def f(lv):
        for name, v in fields.items():
            setattr(lv.tu_arr[_tu_of_block(lv, blk)], name, v)
    return f


# base_level: intra jobs 0 .. 2 on block 0, 3 .. 4 on block 1 (line 1), 5 on block 2; MIP jobs 0 .. 1 on block 0 (8 modes), 2 on block 2 (6 modes); 9 predictions
DEFECTS = [
    ("block width 128", _set("blk_arr", 0, "width", 128)), ("block height 2", _set("blk_arr", 1, "height", 2)), ("block width 12", _set("blk_arr", 0, "width", 12)),
    ("bitDepth 7", _set("blk_arr", 2, "bitDepth", 7)), ("bitDepth 13", _set("blk_arr", 0, "bitDepth", 13)), ("multiRefIdx 3", _set("blk_arr", 1, "multiRefIdx", 3)),
    ("planar off line 0", _set("intra_arr", 3, "mode", 0)), ("mode 67", _set("intra_arr", 1, "mode", 67)),
    ("intra block index past the table", _set("intra_arr", 2, "block", 3)), ("intra block index -1", _set("intra_arr", 0, "block", -1)),
    ("MIP mode 8 of 8", _set("mip_arr", 1, "mode", 8)), ("MIP mode 6 of 6", _set("mip_arr", 2, "mode", 6)), ("MIP transposed 2", _set("mip_arr", 0, "transposed", 2)),
    ("MIP on line 1", _set("mip_arr", 0, "block", 1)), ("MIP block index past the table", _set("mip_arr", 2, "block", 3)),
    ("pred past both tables", _set("tu_arr", 1, "pred", 9)), ("pred -1", _set("tu_arr", 0, "pred", -1)),
    ("qpRem 6", _set("tu_arr", 2, "qpRem", 6)), ("qpRem -1", _set("tu_arr", 2, "qpRem", -1)), ("qpPer -1", _set("tu_arr", 3, "qpPer", -1)),
    ("typeHor 4", _set("tu_arr", 0, "typeHor", 4)), ("typeVer 4", _set("tu_arr", 0, "typeVer", 4)),
    ("TRSKIP with DCT2", _set("tu_arr", 0, "typeHor", lib.TRSKIP)), ("DCT2 with TRSKIP", _set("tu_arr", 0, "typeVer", lib.TRSKIP)),
    ("DST7 on a width of 64", _set_tu_of_block(2, typeHor=lib.DST7)), ("DCT8 on a width of 64", _set_tu_of_block(2, typeHor=lib.DCT8)),
    ("transform skip on 64x16", _set_tu_of_block(2, typeHor=lib.TRSKIP, typeVer=lib.TRSKIP)),
    ("TU reserved", _set("tu_arr", 4, "reserved", 1)), ("TU pad", _set("tu_arr", 4, "pad", 1)), ("block reserved", _set("blk_arr", 1, "reserved", 1, 0)),
    ("intra job reserved", _set("intra_arr", 4, "reserved", 1, 1)), ("MIP job reserved", _set("mip_arr", 1, "reserved", 1, 0)),
]
