"""Restatement of the reference's matrix-based intra prediction (VTM 9.3 CommonLib/MatrixIntraPrediction.cpp: prepareInputForPred :62-118, boundaryDownsampling1D
:163-191, computeReducedPred :283-335, predictionUpsampling / predictionUpsampling1D :194-267; getMipSizeId / getNumModesMip UnitTools.cpp:3873-3900), written after
the reference loop for loop -- the two reduced boundary vectors and their rebasing, the running `weight` pointer with its step back for size id 2, the transposed
copy, and the two 1-D up-sampling passes with the reference's own step / stride arguments on a flat destination (only the orthogonal dimension of a pass is one numpy
expression) -- and independently of vtm_amd/csrc/mip_rules.hpp, which replaces the passes by one closed form per sample.  Plus the case generators and the table
packing (Batch) the GPU tests share; the block helpers are intra_util's."""
import os

import numpy as np

import intra_util as iu
import oracle_lib as ol
from intra_util import POISON, SHAPES25, flog2, make_block, place_in_plane   # noqa: F401

MIP_SHIFT_MATRIX, MIP_OFFSET_MATRIX = 6, 32
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mip.npz")))
    return _golden


def matrices():
    """the three trained matrices as recorded from the reference's MipData.h: flat uint8 arrays"""
    g = golden()
    return g["m4x4"], g["m8x8"], g["m16x16"]


def size_id(w, h):
    if w == 4 and h == 4:
        return 0
    if w == 4 or h == 4 or (w == 8 and h == 8):
        return 1
    return 2


def num_modes(w, h):
    return (16, 8, 6)[size_id(w, h)]


def all_jobs(w, h):
    """the candidate set of estIntraPredLumaQT: every mode, plain then transposed"""
    return [(mode, t) for t in (0, 1) for mode in range(num_modes(w, h))]


def _boundary_downsampling_1d(src, src_len, dst_len):
    dst = [0] * dst_len
    if dst_len < src_len:
        factor = src_len // dst_len
        log2f = flog2(factor)
        rounding = 1 << (log2f - 1)
        src_idx = 0
        for d in range(dst_len):
            s = 0
            for _ in range(factor):
                s += int(src[src_idx])
                src_idx += 1
            dst[d] = (s + rounding) >> log2f
    else:
        for i in range(dst_len):
            dst[i] = int(src[i])
    return dst


def _upsampling_1d(dst, src, src_base, bndry, n_upsmp, n_orth, src_step, src_stride, dst_base, dst_step, dst_stride, bndry_step, factor):
    """predictionUpsampling1D on flat arrays; the loop over idxOrthDim is the numpy axis"""
    log2f = flog2(factor)
    rounding = 1 << (log2f - 1)
    orth = np.arange(n_orth)
    before = bndry[bndry_step - 1 + orth * bndry_step].astype(np.int64)      # bndryLine = bndry + bndryStep - 1, += bndryStep per line
    src_pos, dst_pos = src_base + orth * src_stride, dst_base + orth * dst_stride
    for _ in range(n_upsmp):
        behind = src[src_pos].astype(np.int64)
        scaled_before, scaled_behind = before << log2f, np.zeros(n_orth, np.int64)
        for _pos in range(factor):
            scaled_before = scaled_before - before
            scaled_behind = scaled_behind + behind
            dst[dst_pos] = (scaled_before + scaled_behind + rounding) >> log2f
            dst_pos = dst_pos + dst_step
        before = behind
        src_pos = src_pos + src_step


def predict(top, left, w, h, mode, transposed, bd, mats=None, probe=None):
    """predBlock: the [h, w] int16 prediction.  top / left: the block's lines with index 0 = the corner (only [1 .. w] and [1 .. h] are used).
    probe: a list that receives (min, max) of the reduced prediction before its clip"""
    m4, m8, m16 = matrices() if mats is None else mats
    sid = size_id(w, h)
    bdry, pred_size = (2 if sid == 0 else 4), (4 if sid < 2 else 8)
    up_h, up_v = w // pred_size, h // pred_size
    ref_top, ref_left = np.asarray(top[1:w + 1], np.int64), np.asarray(left[1:h + 1], np.int64)
    # prepareInputForPred
    input_size = 2 * bdry
    top_red, left_red = _boundary_downsampling_1d(ref_top, w, bdry), _boundary_downsampling_1d(ref_left, h, bdry)
    reduced, reduced_t = top_red + left_red, left_red + top_red
    offset, offset_t = reduced[0], reduced_t[0]
    has_first_col = sid < 2
    reduced[0] = ((1 << (bd - 1)) - offset) if has_first_col else 0
    reduced_t[0] = ((1 << (bd - 1)) - offset_t) if has_first_col else 0
    for i in range(1, input_size):
        reduced[i] -= offset
        reduced_t[i] -= offset_t
    # computeReducedPred
    matrix = np.asarray((m4, m8, m16)[sid], np.int64).reshape(-1)
    inp = reduced_t if transposed else reduced
    input_offset = offset_t if transposed else offset
    total = sum(inp)
    off = (1 << (MIP_SHIFT_MATRIX - 1)) - MIP_OFFSET_MATRIX * total
    weight = mode * pred_size * pred_size * (7 if sid == 2 else input_size)           # getMatrixData: &matrix[modeIdx][0][0]
    red_size = sid == 2
    res, max_val = [0] * (pred_size * pred_size), (1 << bd) - 1
    pos_res = 0
    for _y in range(pred_size):
        for _x in range(pred_size):
            if red_size:
                weight -= 1
            tmp = 0 if red_size else inp[0] * int(matrix[weight])
            for i in range(1, input_size):
                tmp += inp[i] * int(matrix[weight + i])
            v = ((tmp + off) >> MIP_SHIFT_MATRIX) + input_offset
            if probe is not None:
                probe.append(v)
            res[pos_res] = min(max(v, 0), max_val)
            pos_res += 1
            weight += input_size
    if transposed:
        res = [res[x * pred_size + y] for y in range(pred_size) for x in range(pred_size)]
    red = np.array(res, np.int64)
    if up_h == 1 and up_v == 1:
        return red.reshape(h, w).astype(np.int16)
    # predictionUpsampling
    dst = np.zeros(w * h, np.int64)
    ver_src, ver_base, ver_step = red, 0, w
    if up_h > 1:
        hor_base = (up_v - 1) * w
        ver_src, ver_base = dst, hor_base
        ver_step *= up_v
        _upsampling_1d(dst, red, 0, ref_left, pred_size, pred_size, 1, pred_size, hor_base, 1, ver_step, up_v, up_h)
    if up_v > 1:
        _upsampling_1d(dst, ver_src, ver_base, ref_top, pred_size, w, ver_step, 1, 0, w, 1, 1, up_v)
    return dst.reshape(h, w).astype(np.int16)


def make_mip_block(rng, w, h, bd, kind, jobs=None):
    """a make_block dict on line 0 whose `modes` are (mode, transposed) pairs, and whose unused line entries (index 0 and everything past W / H) are POISON"""
    b = make_block(rng, w, h, 0, bd, kind, [])
    b["top"], b["left"] = b["top"].copy(), b["left"].copy()
    b["top"][0] = b["left"][0] = POISON
    b["top"][w + 1:] = POISON
    b["left"][h + 1:] = POISON
    b["modes"] = all_jobs(w, h) if jobs is None else list(jobs)
    return b


class Batch:
    """The tables of a list of blocks (make_mip_block dicts) and their jobs in `order` (default: block after block), the lines embedded between runs of POISON.
    exp[k]: the restatement's prediction of job k."""

    def __init__(self, blocks, order=None, fill=0xa5):
        from vtm_amd import lib
        self.lib, self.blocks, self.fill = lib, blocks, fill
        self.ref_buf, ref_offs = iu.embed([(b["top"], b["left"]) for b in blocks])
        self.blk_arr = (lib.IntraBlock * len(blocks))()
        jobs, pred_off = [], 0
        for i, b in enumerate(blocks):
            self.blk_arr[i] = lib.IntraBlock(ref_offs[i], b.get("org_off", 0), b.get("org_stride", 0), b["w"], b["h"], b["bd"], 0)
            for mode, t in b["modes"]:
                jobs.append((i, mode, t, pred_off))
                pred_off += b["w"] * b["h"]
        self.pred_len = pred_off
        self.jobs = [jobs[k] for k in order] if order is not None else jobs
        self.n = len(self.jobs)
        self.job_arr = (lib.MipJob * max(self.n, 1))(*[lib.MipJob(off, i, mode, t) for i, mode, t, off in self.jobs])
        self._exp, self.probe = None, []      # probe: the unclipped reduced samples of every job

    @property
    def exp(self):
        if self._exp is None:
            self._exp = [predict(self.blocks[i]["top"], self.blocks[i]["left"], self.blocks[i]["w"], self.blocks[i]["h"], mode, t, self.blocks[i]["bd"], probe=self.probe)
                         for i, mode, t, _ in self.jobs]
        return self._exp

    def _upload(self, ctx):
        from vtm_amd.device import struct_array_to_numpy
        return ctx.to_device(self.ref_buf), ctx.to_device(struct_array_to_numpy(self.blk_arr)), ctx.to_device(struct_array_to_numpy(self.job_arr))

    def run_pred(self, ctx, keep=False):
        """-> the flat int16 prediction buffer (pre-filled with the fill byte), or the device buffers too"""
        d_ref, d_blk, d_job = self._upload(ctx)
        d_pred = ctx.to_device(np.full(max(self.pred_len, 1) * 2, self.fill, np.uint8))
        ctx.mip_pred_batch(d_ref.ptr, d_blk.ptr, len(self.blocks), d_job.ptr, self.n, d_pred.ptr)
        ctx.sync()
        flat = d_pred.to_host(np.int16, shape=(-1,))
        if keep:
            return flat, (d_ref, d_blk, d_job, d_pred)
        for b in (d_ref, d_blk, d_job, d_pred):
            b.free()
        return flat

    def check_pred(self, flat, skip=()):
        for k, (i, mode, t, off) in enumerate(self.jobs):
            if k in skip:
                continue
            b = self.blocks[i]
            got = flat[off:off + b["w"] * b["h"]].reshape(b["h"], b["w"])
            assert np.array_equal(got, self.exp[k]), (k, b["w"], b["h"], mode, t, b["bd"], np.argwhere(got != self.exp[k])[:4].tolist())

    def run_presel(self, ctx, plane):
        d_ref, d_blk, d_job = self._upload(ctx)
        d_org = ctx.to_device(plane)
        d_out = ctx.to_device(np.full(max(self.n, 1) * 16, self.fill, np.uint8))
        ctx.mip_presel_batch(d_ref.ptr, d_org.ptr, d_blk.ptr, len(self.blocks), d_job.ptr, self.n, d_out.ptr)
        ctx.sync()
        res = d_out.to_host(np.uint64, shape=(-1, 2))
        for b in (d_ref, d_blk, d_job, d_org, d_out):
            b.free()
        return res

    def exp_dist(self, plane):
        """[n, 2] (SAD, SATD) of the restatement's predictions through the oracle's distortions"""
        out = np.zeros((self.n, 2), np.uint64)
        for k, (i, _, _, _) in enumerate(self.jobs):
            b = self.blocks[i]
            x, y = b["org_xy"]
            org = ol.i16(plane[y:y + b["h"], x:x + b["w"]])
            out[k] = (ol.o_dist(0, org, ol.i16(self.exp[k]), b["w"], b["h"]), ol.o_dist(1, org, ol.i16(self.exp[k]), b["w"], b["h"]))
        return out
