"""Tables, buffers and expectations of the intra chroma residual chain (vtmhip_intra_chroma_chain_batch_dev) for the CPU and GPU tests.

A Level is a list of cclm_util.make_block dicts with their `modes` placed in an original plane (cclm_util.place_orgs), a list of single specs
(pred, component, ts, qp, irap, adj) and a list of joint specs (pred, cbfMask, signFlag, ts, qp, irap, adj).  Predictions are numbered as the job table numbers them.
Every prediction and output block lies between GAP samples of fill, at offsets that are only 2-byte aligned; the Cb reconstruction of a joint job shares its buffer
with the single jobs' reconstructions, the Cr reconstruction has a buffer of its own."""
import numpy as np

import cclm_util as cu
import lmcs_util as lu
from vtm_amd import lib
from vtm_amd.lib import IntraChromaJointJob, IntraChromaTuJob, JccrJob, JccrResult, TuJob, TuResult

GAP = 5
FILL = 0xa5
FILL16 = np.frombuffer(bytes([FILL, FILL]), np.int16)[0]
FILL32 = np.frombuffer(bytes([FILL] * 4), np.int32)[0]
TU_FIELDS = [f for f, _ in TuJob._fields_]
JCCR_FIELDS = ["cbOff", "crOff", "outOff", "resiStride", "width", "height", "qpPer", "qpRem", "typeHor", "bitDepth", "isIRAP", "cbfMask", "signFlag", "reserved0",
               "chromaAdj"]
RES_DT = np.dtype([("sse", "<u8"), ("sseResi", "<u8"), ("sumAbs", "<i4"), ("absSum", "<i4")])
JRES_DT = np.dtype([("sseCb", "<u8"), ("sseCr", "<u8"), ("sseResiCb", "<u8"), ("sseResiCr", "<u8"), ("fwdDist", "<i8"), ("sumAbs", "<i4"), ("absSum", "<i4")])
ADJS = (0, 1500, 2048, 3277, 5000)


def qp_of(qp, bd, ts=False):
    """QpParam::per / rem of a base QP at this bit depth (Quant.cpp:65-104); transform skip: the floor of 4 on the base QP"""
    base = qp + 6 * (bd - 8)
    return divmod(max(base, 4) if ts else base, 6)


def _plan(sizes, ts):
    mw, mh = max([w for w, _ in sizes] + [0]), max([h for _, h in sizes] + [0])
    return mw, mh, int(len(sizes) == 1 and not ts)


def expand(blocks, jobs, tu_jobs, joint_jobs):
    """the Python restatement of vtmhip_intra_chroma_chain_make_jobs over ctypes records:
    ([dict of every vtmhip_tu_job field], [dict of every vtmhip_jccr_job field], (maxWidth, maxHeight, uniform) of the single jobs, of the joint jobs, crs)"""
    out_tu, out_joint, sizes, ts, crs = [], [], [set(), set()], [False, False], 0
    for t in tu_jobs:
        j = jobs[t.pred]
        b = blocks[j.block]
        out_tu.append(dict(resiOff=j.crPredOff if t.component else j.cbPredOff, outOff=t.outOff, resiStride=b.width, width=b.width, height=b.height, qpPer=t.qpPer,
                           qpRem=t.qpRem, typeHor=t.typeHor, typeVer=t.typeHor, bitDepth=b.bitDepth, isIRAP=t.isIRAP, pad=0, chromaAdj=t.chromaAdj))
        sizes[0].add((b.width, b.height))
        ts[0] |= t.typeHor == lib.TRSKIP
        crs |= int(t.chromaAdj != 0)
    for t in joint_jobs:
        j = jobs[t.pred]
        b = blocks[j.block]
        out_joint.append(dict(cbOff=j.cbPredOff, crOff=j.crPredOff, outOff=t.outOff, resiStride=b.width, width=b.width, height=b.height, qpPer=t.qpPer, qpRem=t.qpRem,
                              typeHor=t.typeHor, bitDepth=b.bitDepth, isIRAP=t.isIRAP, cbfMask=t.cbfMask, signFlag=t.signFlag, reserved0=0, chromaAdj=t.chromaAdj,
                              reserved1=[0, 0, 0, 0]))
        sizes[1].add((b.width, b.height))
        ts[1] |= t.typeHor == lib.TRSKIP
        crs |= int(t.chromaAdj != 0)
    return out_tu, out_joint, _plan(sizes[0], ts[0]), _plan(sizes[1], ts[1]), crs


def tu_fields(j):
    return {f: getattr(j, f) for f in TU_FIELDS}


def jccr_fields(j):
    return dict({f: getattr(j, f) for f in JCCR_FIELDS}, reserved1=list(j.reserved1))


def _jccr_record(d):
    j = JccrJob()
    for f in JCCR_FIELDS:
        setattr(j, f, d[f])
    return j


class Level:
    def __init__(self, blocks, plane, singles, joints, order=None, job_order=None):
        """order: (permutation of the single specs, permutation of the joint specs) or None; job_order: a permutation of the prediction jobs (the specs name
        predictions by their position in the permuted table)"""
        self.blocks, self.plane = blocks, plane
        self.batch = cu.Batch(blocks, order=job_order, fill=FILL)      # the reference lines between runs of 0x7fff, the luma planes, the block table
        self.ref_buf, self.luma_buf, self.blk_arr, self.job_arr = self.batch.ref_buf, self.batch.luma_buf, self.batch.blk_arr, self.batch.job_arr
        self.n_pred, off, self.preds = self.batch.n, GAP, []
        for k, (i, _, _) in enumerate(self.batch.jobs):
            n = blocks[i]["w"] * blocks[i]["h"]
            self.job_arr[k].cbPredOff, self.job_arr[k].crPredOff = off, off + n + GAP
            self.preds.append((i, off, off + n + GAP))                  # prediction p -> (block, cbPredOff, crPredOff)
            off += 2 * (n + GAP)
        self.pred_len = off
        if order is not None:
            singles, joints = [singles[k] for k in order[0]], [joints[k] for k in order[1]]
        self.singles, self.joints, off, tu, jt = list(singles), list(joints), GAP, [], []
        for p, comp, ts, qp, irap, adj in self.singles:
            b = blocks[self.preds[p][0]]
            per, rem = qp_of(qp, b["bd"], ts)
            tu.append(IntraChromaTuJob(off, p, per, rem, comp, lib.TRSKIP if ts else lib.DCT2, irap, 0, adj, 0))
            off += b["w"] * b["h"] + GAP
        for p, mask, sign, ts, qp, irap, adj in self.joints:
            b = blocks[self.preds[p][0]]
            per, rem = qp_of(qp, b["bd"], ts)
            jt.append(IntraChromaJointJob(off, p, per, rem, lib.TRSKIP if ts else lib.DCT2, irap, mask, sign, adj, 0))
            off += b["w"] * b["h"] + GAP
        self.out_len, self.n_tu, self.n_joint = off, len(tu), len(jt)
        self.tu_arr, self.joint_arr = (IntraChromaTuJob * max(len(tu), 1))(*tu), (IntraChromaJointJob * max(len(jt), 1))(*jt)
        self._exp = None

    def block_of_pred(self, p):
        return self.blocks[self.preds[p][0]]

    def org_of(self, b, c):
        x, y = b["org_xy"][c]
        return self.plane[y:y + b["h"], x:x + b["w"]].astype(np.int64)

    def tables(self):
        return self.blk_arr, self.job_arr, [self.tu_arr[k] for k in range(self.n_tu)], [self.joint_arr[k] for k in range(self.n_joint)]

    def chain_jobs(self):
        """the restatement's expansion as ctypes arrays: (TuJob array, JccrJob array, single plan, joint plan, crs)"""
        tu, jt, pt, pj, crs = expand(*self.tables())
        return ((TuJob * max(self.n_tu, 1))(*[TuJob(*[j[f] for f in TU_FIELDS]) for j in tu]), (JccrJob * max(self.n_joint, 1))(*[_jccr_record(j) for j in jt]), pt, pj, crs)

    def paths(self):
        """what the host plan of this level reaches: (lanes per prediction, single chain path, joint chain path, finish lanes, crs)"""
        _, _, pt, pj, crs = self.chain_jobs()
        lanes = 16 if max(b["w"] * b["h"] for b in self.blocks) <= 64 else 64

        def tu_path(n, mw, mh, uni):
            if n == 0:
                return None
            if not uni and n >= 256 and min(mw, mh) >= 8:
                return "bucketed"
            if uni:
                return "lane" if mw * mh <= 32 else "blocked" if min(mw, mh) >= 8 else "generic64" if mw * mh <= 256 else "generic256"
            return "generic64" if mw * mh <= 256 else "generic256"

        def joint_path(n, mw, mh, uni):
            if n == 0:
                return None
            if uni:
                return "lane" if mw * mh <= 32 else "blocked" if min(mw, mh) >= 8 else "generic64" if mw * mh <= 256 else "generic256"
            return "generic64" if mw * mh <= 256 else "generic256"

        area = max([self.block_of_pred(s[0])["w"] * self.block_of_pred(s[0])["h"] for s in self.singles + self.joints] + [0])
        return lanes, tu_path(self.n_tu, *pt), joint_path(self.n_joint, *pj), 16 if area <= 256 else 64, crs

    def device_args(self, ctx, levels=True, luma=True, n_pred=None, n_tu=None, n_joint=None):
        """the tables uploaded and the seven output buffers pre-filled with FILL: (the arguments of Context.intra_chroma_chain_batch in order, inputs, outputs)"""
        from vtm_amd.device import struct_array_to_numpy as s2n
        n_pred, n_tu, n_joint = (self.n_pred if n_pred is None else n_pred), (self.n_tu if n_tu is None else n_tu), (self.n_joint if n_joint is None else n_joint)
        ins = [ctx.to_device(a) for a in (self.ref_buf, self.luma_buf, self.plane, s2n(self.blk_arr), s2n(self.job_arr), s2n(self.tu_arr), s2n(self.joint_arr))]
        outs = [ctx.to_device(np.full(n, FILL, np.uint8)) for n in (2 * self.pred_len, 2 * self.pred_len, 2 * self.out_len, 2 * self.out_len, 24 * max(self.n_tu, 1),
                                                                    48 * max(self.n_joint, 1), 4 * self.out_len)]
        args = [ins[0].ptr, ins[1].ptr if luma else None, ins[2].ptr, ins[3].ptr, len(self.blocks), ins[4].ptr, n_pred, ins[5].ptr, n_tu, ins[6].ptr, n_joint,
                outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[4].ptr, outs[5].ptr, outs[6].ptr if levels else None]
        return args, ins, outs

    @staticmethod
    def read(outs):
        return dict(pred=outs[0].to_host(np.int16, shape=(-1,)), resi=outs[1].to_host(np.int16, shape=(-1,)), reco=outs[2].to_host(np.int16, shape=(-1,)),
                    recoCr=outs[3].to_host(np.int16, shape=(-1,)), results=np.frombuffer(outs[4].to_host(np.uint8, shape=(-1,)).tobytes(), RES_DT),
                    jres=np.frombuffer(outs[5].to_host(np.uint8, shape=(-1,)).tobytes(), JRES_DT), levels=outs[6].to_host(np.int32, shape=(-1,)))

    # ---- the device call ----------------------------------------------------------------------------------------------------------------------------------
    def run(self, ctx, **kw):
        """-> dict of the seven output buffers as numpy arrays, every one pre-filled with FILL, and the status"""
        args, ins, outs = self.device_args(ctx, **kw)
        status = lib.OK
        try:
            ctx.intra_chroma_chain_batch(*args)
        except lib.VtmHipError as e:
            status = e.status
        ctx.sync()
        got = dict(self.read(outs), status=status)
        for b in ins + outs:
            b.free()
        return got

    # ---- expectation A: entries that are pinned to the reference, numpy between them ---------------------------------------------------------------------------
    def expect(self, ctx):
        if self._exp is not None:
            return self._exp
        from vtm_amd.device import struct_array_to_numpy as s2n
        bufs = [ctx.to_device(a) for a in (self.ref_buf, self.luma_buf, s2n(self.blk_arr), s2n(self.job_arr))]
        d_pred = ctx.to_device(np.full(2 * self.pred_len, FILL, np.uint8))
        ctx.intra_chroma_pred_batch(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, len(self.blocks), bufs[3].ptr, self.n_pred, d_pred.ptr)
        ctx.sync()
        pred = d_pred.to_host(np.int16, shape=(-1,))
        bufs.append(d_pred)
        resi = np.full(self.pred_len, FILL16, np.int16)
        for i, cb, cr in self.preds:
            b = self.blocks[i]
            n = b["w"] * b["h"]
            for c, off in ((0, cb), (1, cr)):
                resi[off:off + n] = (self.org_of(b, c).reshape(-1) - pred[off:off + n]).astype(np.int16)
        levels = np.full(self.out_len, FILL32, np.int32)
        reco, reco_cr = np.full(self.out_len, FILL16, np.int16), np.full(self.out_len, FILL16, np.int16)
        results, jres, clipped = [], [], [0, 0]
        tu, jt, pt, pj, _ = self.chain_jobs()
        d_resi, d_lev, d_rec, d_rec_cr = ctx.to_device(resi), ctx.to_device(levels), ctx.to_device(reco), ctx.to_device(reco_cr)
        bufs += [d_resi, d_lev, d_rec, d_rec_cr]
        tres = jr = None
        if self.n_tu:
            d_jobs, d_res = ctx.to_device(s2n(tu)), ctx.alloc(16 * self.n_tu)
            ctx.tu_chain_crs_batch(d_resi.ptr, d_jobs.ptr, self.n_tu, pt[0], pt[1], d_res.ptr, d_lev.ptr, d_rec.ptr, uniform=False)
            ctx.sync()
            tres = (TuResult * self.n_tu).from_buffer_copy(d_res.to_host(np.uint8, shape=(-1,)).tobytes())
            bufs += [d_jobs, d_res]
        if self.n_joint:
            d_jobs, d_res = ctx.to_device(s2n(jt)), ctx.alloc(32 * self.n_joint)
            ctx.jccr_chain_crs_batch(d_resi.ptr, d_jobs.ptr, self.n_joint, pj[0], pj[1], d_res.ptr, d_lev.ptr, d_rec.ptr, d_rec_cr.ptr, uniform=False)
            ctx.sync()
            jr = (JccrResult * self.n_joint).from_buffer_copy(d_res.to_host(np.uint8, shape=(-1,)).tobytes())
            bufs += [d_jobs, d_res]
        levels, reco, reco_cr = d_lev.to_host(np.int32, shape=(-1,)), d_rec.to_host(np.int16, shape=(-1,)).copy(), d_rec_cr.to_host(np.int16, shape=(-1,)).copy()

        def finish(buf, out_off, b, c, pred_off):
            n, mx = b["w"] * b["h"], (1 << b["bd"]) - 1
            raw = pred[pred_off:pred_off + n].astype(np.int64) + buf[out_off:out_off + n]
            rec = np.clip(raw, 0, mx)
            clipped[0] += int((raw < 0).sum())
            clipped[1] += int((raw > mx).sum())
            buf[out_off:out_off + n] = rec
            d = self.org_of(b, c).reshape(-1) - rec
            return int((d * d).sum())

        for k in range(self.n_tu):
            t = self.tu_arr[k]
            i, cb, cr = self.preds[t.pred]
            sse = finish(reco, t.outOff, self.blocks[i], t.component, cr if t.component else cb)
            results.append((sse, int(tres[k].sse), int(tres[k].sumAbs), int(tres[k].absSum)))
        for k in range(self.n_joint):
            t = self.joint_arr[k]
            i, cb, cr = self.preds[t.pred]
            sse_cb, sse_cr = finish(reco, t.outOff, self.blocks[i], 0, cb), finish(reco_cr, t.outOff, self.blocks[i], 1, cr)
            jres.append((sse_cb, sse_cr, int(jr[k].sseCb), int(jr[k].sseCr), int(jr[k].fwdDist), int(jr[k].sumAbs), int(jr[k].absSum)))
        for b in bufs:
            b.free()
        self._exp = dict(pred=pred, resi=resi, levels=levels, reco=reco, recoCr=reco_cr, results=results, jres=jres, clipped=clipped)
        return self._exp

    def check(self, got, exp, levels=True):
        """every buffer in full: the blocks and the fill between them"""
        assert got["status"] == lib.OK
        for key in ("pred", "resi", "reco", "recoCr") + (("levels",) if levels else ()):
            assert np.array_equal(got[key], exp[key]), (key, np.argwhere(got[key] != exp[key])[:6].tolist())
        if not levels:
            assert (got["levels"] == FILL32).all()
        res = [tuple(int(v) for v in r) for r in got["results"][:self.n_tu]]
        assert res == exp["results"], [(k, a, b) for k, (a, b) in enumerate(zip(res, exp["results"])) if a != b][:4]
        res = [tuple(int(v) for v in r) for r in got["jres"][:self.n_joint]]
        assert res == exp["jres"], [(k, a, b) for k, (a, b) in enumerate(zip(res, exp["jres"])) if a != b][:4]
        if not self.n_tu:
            assert (got["results"].view(np.uint8) == FILL).all()
        if not self.n_joint:
            assert (got["jres"].view(np.uint8) == FILL).all() and (got["recoCr"] == FILL16).all()

    @staticmethod
    def untouched(got):
        return all((got[k].view(np.uint8) == FILL).all() for k in ("pred", "resi", "levels", "reco", "recoCr", "results", "jres"))

    # ---- expectation B: without any device entry -- cclm_util's predictions, lmcs_util's chains on the CPU oracle ------------------------------------------------
    def _oracle_pred(self, p):
        i, _, _ = self.preds[p]
        b = self.blocks[i]
        return b, self.batch.exp[p].astype(np.int64), [self.org_of(b, c) for c in (0, 1)]

    def oracle_single(self, k):
        """single job k: dict(pred, resi, levels, reco, raw, result)"""
        t = self.tu_arr[k]
        b, pred, org = self._oracle_pred(t.pred)
        c = t.component
        resi = np.ascontiguousarray(org[c] - pred[c], np.int16)
        e = lu.tu_chain_expect(resi, t.chromaAdj, b["bd"], t.qpPer, t.qpRem, t.isIRAP, int(t.typeHor == lib.TRSKIP))
        raw = pred[c] + e["rec"].reshape(pred[c].shape)
        reco = np.clip(raw, 0, (1 << b["bd"]) - 1)
        d = org[c] - reco
        return dict(pred=pred[c].reshape(-1), resi=resi.reshape(-1), levels=e["levels"], reco=reco.reshape(-1), raw=raw, result=(int((d * d).sum()), e["sse"], e["sumAbs"], e["absSum"]))

    def oracle_joint(self, k):
        """joint job k: dict(levels, recoCb, recoCr, raw, result)"""
        t = self.joint_arr[k]
        b, pred, org = self._oracle_pred(t.pred)
        cb, cr = (np.ascontiguousarray(org[c] - pred[c], np.int16) for c in (0, 1))
        e = lu.jccr_chain_expect(cb, cr, t.chromaAdj, t.cbfMask, t.signFlag, b["bd"], t.qpPer, t.qpRem, t.isIRAP, int(t.typeHor == lib.TRSKIP))
        raw = [pred[0] + e["recCb"].reshape(cb.shape), pred[1] + e["recCr"].reshape(cb.shape)]
        reco = [np.clip(r, 0, (1 << b["bd"]) - 1) for r in raw]
        sse = [int(((org[c] - reco[c]) ** 2).sum()) for c in (0, 1)]
        return dict(levels=e["levels"], recoCb=reco[0].reshape(-1), recoCr=reco[1].reshape(-1), raw=raw,
                    result=(sse[0], sse[1], e["sseCb"], e["sseCr"], e["fwdDist"], e["sumAbs"], e["absSum"]))

    def check_oracle_single(self, got, k):
        t, e = self.tu_arr[k], self.oracle_single(k)
        i, cb, cr = self.preds[t.pred]
        n, po = self.blocks[i]["w"] * self.blocks[i]["h"], cr if t.component else cb
        assert np.array_equal(got["pred"][po:po + n], e["pred"]) and np.array_equal(got["resi"][po:po + n], e["resi"]), k
        assert np.array_equal(got["levels"][t.outOff:t.outOff + n], e["levels"]) and np.array_equal(got["reco"][t.outOff:t.outOff + n], e["reco"]), k
        assert tuple(int(v) for v in got["results"][k]) == e["result"], (k, got["results"][k], e["result"])

    def check_oracle_joint(self, got, k):
        t, e = self.joint_arr[k], self.oracle_joint(k)
        n = self.block_of_pred(t.pred)["w"] * self.block_of_pred(t.pred)["h"]
        assert np.array_equal(got["levels"][t.outOff:t.outOff + n], e["levels"]), k
        assert np.array_equal(got["reco"][t.outOff:t.outOff + n], e["recoCb"]) and np.array_equal(got["recoCr"][t.outOff:t.outOff + n], e["recoCr"]), k
        assert tuple(int(v) for v in got["jres"][k]) == e["result"], (k, got["jres"][k], e["result"])


def make_blocks(rng, shapes, stride=97):
    """shapes: (w, h, bd, kind, availability class, colocated, first row, modes) per block -> (blocks, the Cb / Cr original plane)"""
    blocks = [cu.make_block(rng, w, h, bd, kind, cls, coloc=coloc, first_row=first, modes=modes, k=k) for k, (w, h, bd, kind, cls, coloc, first, modes) in enumerate(shapes)]
    for b, s in zip(blocks, shapes):
        b["kind"] = s[3]
    plane = cu.place_orgs(rng, blocks, stride)
    for b in blocks:
        if b["kind"] == "const":           # constant lines and luma: every prediction is (nearly) constant; an original within 1 of it quantises to nothing
            for c in (0, 1):
                (x, y), v = b["org_xy"][c], int(b["lines"][c][0][1])
                plane[y:y + b["h"], x:x + b["w"]] = np.clip(v + rng.integers(-1, 2, (b["h"], b["w"])), 0, (1 << b["bd"]) - 1)
    return blocks, plane


def make_level(rng, shapes, cands_of, stride=97, order=None, job_order=None):
    """cands_of( p, block dict ) -> (the (component, ts, qp, irap, adj) single candidates, the (cbfMask, signFlag, ts, qp, irap, adj) joint candidates) of prediction p"""
    blocks, plane = make_blocks(rng, shapes, stride)
    preds = [i for i, b in enumerate(blocks) for _ in b["modes"]]
    if job_order is not None:
        preds = [preds[k] for k in job_order]
    singles, joints = [], []
    for p, i in enumerate(preds):
        s, j = cands_of(p, blocks[i])
        singles += [(p,) + tuple(c) for c in s]
        joints += [(p,) + tuple(c) for c in j]
    return Level(blocks, plane, singles, joints, order, job_order)


# ---- malformed tables: one defect each, applied to a fresh base_level ---------------------------------------------------------------------------------------------
def base_level(seed=5):
    """three blocks (8x8 with LM, 16x4, 32x16 with MDLM_T), two or three predictions each; per prediction Cb DCT2, Cr transform skip and two joint candidates"""
    shapes = [(8, 8, 10, "random", "full", False, False, [0, 67, 50]), (16, 4, 8, "random", "both", True, False, [1, 18]), (32, 16, 12, "random", "above", False, True, [34, 69])]
    return make_level(np.random.default_rng(seed), shapes, lambda p, b: ([(0, 0, 30, p & 1, 3277), (1, 1, 27, 0, 0)], [(1 + p % 3, p & 1, 0, 30, 0, 3277), (3, 0, 1, 33, 1, 2048)]))


def _set(table, k, field, v, idx=None):
    def f(lv):
        rec = getattr(lv, table)[k]
        if idx is None:
            setattr(rec, field, v)
        else:
            getattr(rec, field)[idx] = v
    return f


# base_level: predictions 0 .. 2 on block 0, 3 .. 4 on block 1, 5 .. 6 on block 2; 14 single and 14 joint jobs
DEFECTS = [
    ("block width 64", _set("blk_arr", 0, "width", 64)), ("block height 2", _set("blk_arr", 1, "height", 2)), ("block width 12", _set("blk_arr", 0, "width", 12)),
    ("bitDepth 7", _set("blk_arr", 2, "bitDepth", 7)), ("bitDepth 13", _set("blk_arr", 0, "bitDepth", 13)), ("above 2", _set("blk_arr", 1, "above", 2)),
    ("firstRow 2", _set("blk_arr", 0, "firstRow", 2)), ("colocated 2", _set("blk_arr", 2, "colocated", 2)),
    ("aboveRight without above", lambda lv: (_set("blk_arr", 1, "above", 0)(lv), _set("blk_arr", 1, "aboveRight", 2)(lv))),
    ("belowLeft odd", _set("blk_arr", 0, "belowLeft", 3)), ("belowLeft beyond the side", _set("blk_arr", 0, "belowLeft", 10)), ("aboveRight -2", _set("blk_arr", 0, "aboveRight", -2)),
    ("block reserved", _set("blk_arr", 1, "reserved", 1, 2)),
    ("mode 70", _set("job_arr", 1, "mode", 70)), ("block index past the table", _set("job_arr", 2, "block", 3)), ("block index -1", _set("job_arr", 0, "block", -1)),
    ("job reserved", _set("job_arr", 4, "reserved", 1, 1)),
    ("single pred past the table", _set("tu_arr", 1, "pred", 7)), ("single pred -1", _set("tu_arr", 0, "pred", -1)), ("component 2", _set("tu_arr", 3, "component", 2)),
    ("single typeHor DST7", _set("tu_arr", 0, "typeHor", lib.DST7)), ("single typeHor 4", _set("tu_arr", 2, "typeHor", 4)),
    ("single qpRem 6", _set("tu_arr", 2, "qpRem", 6)), ("single qpRem -1", _set("tu_arr", 2, "qpRem", -1)), ("single qpPer -1", _set("tu_arr", 3, "qpPer", -1)),
    ("single chromaAdj 32768", _set("tu_arr", 4, "chromaAdj", 32768)), ("single reserved", _set("tu_arr", 4, "reserved", 1)), ("single pad", _set("tu_arr", 5, "pad", 1)),
    ("joint pred past the table", _set("joint_arr", 1, "pred", 7)), ("joint pred -1", _set("joint_arr", 13, "pred", -1)),
    ("cbfMask 0", _set("joint_arr", 0, "cbfMask", 0)), ("cbfMask 4", _set("joint_arr", 2, "cbfMask", 4)), ("signFlag 2", _set("joint_arr", 3, "signFlag", 2)),
    ("joint typeHor DCT8", _set("joint_arr", 0, "typeHor", lib.DCT8)), ("joint qpRem 6", _set("joint_arr", 5, "qpRem", 6)), ("joint qpPer -1", _set("joint_arr", 6, "qpPer", -1)),
    ("joint chromaAdj 40000", _set("joint_arr", 7, "chromaAdj", 40000)), ("joint pad", _set("joint_arr", 8, "pad", 1)),
]
