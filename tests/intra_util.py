"""Numpy restatement of the reference's luma intra prediction (VTM 9.3 CommonLib/IntraPrediction.cpp: initPredIntraParams :356-444, xFilterReferenceSamples
:1166-1200, xGetPredValDc :153-182, xPredIntraPlanar :294-348, xPredIntraAng :459-643, the PDPC of predIntraAng :244-265) for a luma block without ISP, MIP or
BDPCM, written after the reference loop for loop -- the extended main reference is built as an array, the rows advance by `deltaPos += intraPredAngle`, planar
accumulates its row and column sums, horizontal modes predict the transposed block and flip it -- and independently of vtm_amd/csrc/intra_rules.hpp, which replaces
the recurrences by closed forms.  A row is one numpy expression.  Plus the case generators and the table packing (Batch) the GPU tests share."""
import ctypes as C

import numpy as np

import oracle_lib as ol

PLANAR, DC, HOR, DIA, VER, VDIA, NUM_MODES = 0, 1, 18, 34, 50, 66, 67
SIDES = (4, 8, 16, 32, 64)
SHAPES25 = [(w, h) for w in SIDES for h in SIDES]
ANG_TABLE = [0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32, 35, 39, 45, 51, 57, 64, 73, 86, 102, 128, 171, 256, 341, 512, 1024]
INV_ANG_TABLE = [0, 16384, 8192, 5461, 4096, 2731, 2048, 1638, 1365, 1170, 1024, 910, 819, 712, 630, 565, 512, 468, 420, 364, 321, 287, 256, 224, 191, 161, 128, 96,
                 64, 48, 32, 16]
INTRA_FILTER = [24, 24, 24, 14, 2, 0, 0, 0]     # m_aucIntraFilter
MODE_SHIFT = [0, 6, 10, 12, 14, 15]
PARAM_FIELDS = ("predMode", "isModeVer", "intraPredAngle", "invAngle", "angularScale", "applyPDPC", "refFilterFlag", "interpolationFlag")
POISON = 0x7fff

_cubic = None


def cubic_taps():
    """InterpolationFilter::getChromaFilterTable: the oracle's copy (pinned to the reference's by tests/test_oracle_vs_ref.py)"""
    global _cubic
    if _cubic is None:
        arr = (C.c_int16 * 128).in_dll(ol.oracle(), "vo_chroma_filter")
        _cubic = np.array(arr, dtype=np.int64).reshape(32, 4)
    return _cubic


def flog2(v):
    return int(v).bit_length() - 1


def wide_angle(w, h, mode):
    if DC < mode <= VDIA:
        delta = abs(flog2(w) - flog2(h))
        if w > h and mode < 2 + MODE_SHIFT[delta]:
            mode += VDIA - 1
        elif h > w and mode > VDIA - MODE_SHIFT[delta]:
            mode -= VDIA - 1
    return mode


def params(w, h, mode, m):
    """m_ipaParam after initPredIntraParams as a dict of PARAM_FIELDS (angularScale: 0 where the reference does not set it)"""
    pred_mode = wide_angle(w, h, mode)
    p = dict(predMode=pred_mode, isModeVer=int(pred_mode >= DIA), intraPredAngle=0, invAngle=0, angularScale=0, applyPDPC=int(w >= 4 and h >= 4 and m == 0),
             refFilterFlag=0, interpolationFlag=0)
    ang_mode = pred_mode - VER if p["isModeVer"] else -(pred_mode - HOR)
    abs_ang = 0
    if DC < mode < NUM_MODES:
        abs_ang = ANG_TABLE[abs(ang_mode)]
        p["invAngle"] = INV_ANG_TABLE[abs(ang_mode)]
        p["intraPredAngle"] = -abs_ang if ang_mode < 0 else abs_ang
        if ang_mode < 0:
            p["applyPDPC"] = 0
        elif ang_mode > 0:
            side = h if p["isModeVer"] else w
            p["angularScale"] = min(2, flog2(side) - (flog2(3 * p["invAngle"] - 2) - 8))
            p["applyPDPC"] &= int(p["angularScale"] >= 0)
    if m or mode == DC:
        pass
    elif mode == PLANAR:
        p["refFilterFlag"] = int(w * h > 32)
    else:
        diff = min(abs(pred_mode - HOR), abs(pred_mode - VER))
        if diff > INTRA_FILTER[(flog2(w) + flog2(h)) >> 1]:
            integer = (abs_ang & 31) == 0
            assert w * h > 32
            p["refFilterFlag"], p["interpolationFlag"] = int(integer), int(not integer)
    return p


def filter_lines(top, left):
    """xFilterReferenceSamples on the two lines (m = 0): the corner from the first two samples of both, [1 2 1] inside, the last sample copied"""
    out = []
    corner = (int(top[0]) + int(top[1]) + int(left[0]) + int(left[1]) + 2) >> 2
    for u in (top.astype(np.int64), left.astype(np.int64)):
        f = u.copy()
        f[0] = corner
        f[1:-1] = (u[:-2] + 2 * u[1:-1] + u[2:] + 2) >> 2
        out.append(f)
    return out


def _pel(a):
    """through Pel: the wrap of an int16 store"""
    return ((np.asarray(a, np.int64) + 32768) & 0xffff) - 32768


def _planar(top, left, w, h):
    lw, lh = flog2(w), flog2(h)
    top_row, left_col = top[1:w + 2].copy(), left[1:h + 2].copy()
    bottom_left, top_right = left_col[h], top_row[w]
    bottom_row = bottom_left - top_row[:w]
    top_row = top_row[:w] << lh
    right_col = top_right - left_col[:h]
    left_col = left_col[:h] << lw
    pred = np.zeros((h, w), np.int64)
    for y in range(h):
        hor = left_col[y] + np.cumsum(np.full(w, right_col[y]))      # horPred += rightColumn[y], per x
        top_row = top_row + bottom_row                                # topRow[x] += bottomRow[x], per row
        pred[y] = ((hor << lh) + (top_row << lw) + (1 << (lw + lh))) >> (1 + lw + lh)
    return _pel(pred)


def _dc(top, left, w, h, m):
    denom = w << 1 if w == h else max(w, h)
    s = 0
    if w >= h:
        s += int(top[m + 1:m + 1 + w].sum())
    if w <= h:
        s += int(left[m + 1:m + 1 + h].sum())
    return (s + (denom >> 1)) >> flog2(denom)


def _angular(p, top, left, w, h, m, max_val, probe=None):
    ver, angle, inv = bool(p["isModeVer"]), p["intraPredAngle"], p["invAngle"]
    off = 64 + 8                                       # room for the negative extension
    ref_above, ref_left = np.zeros(2 * 64 + 3 + 33 * 2 + off, np.int64), np.zeros(2 * 64 + 3 + 33 * 2 + off, np.int64)
    if angle < 0:
        ref_above[off:off + w + 2 + m] = top[:w + 2 + m]
        ref_left[off:off + h + 2 + m] = left[:h + 2 + m]
        main, side = (ref_above, ref_left) if ver else (ref_left, ref_above)
        size_side = h if ver else w
        for k in range(-size_side, 0):
            main[off + k] = side[off + min((-k * inv + 256) >> 9, size_side)]
    else:
        ref_above[off:off + 2 * w + 1 + m] = top
        ref_left[off:off + 2 * h + 1 + m] = left
        main, side = (ref_above, ref_left) if ver else (ref_left, ref_above)
        log2_ratio = flog2(w) - flog2(h)
        s = max(0, log2_ratio if ver else -log2_ratio)
        max_index = (m << s) + 2
        ref_length = 2 * w if ver else 2 * h
        main[off + ref_length + m + 1:off + ref_length + m + 1 + max_index] = main[off + ref_length + m]
    if not ver:
        w, h = h, w
    base = off + m                                     # refMain += multiRefIdx, refSide += multiRefIdx
    dst = np.zeros((h, w), np.int64)
    xs = np.arange(w)
    if angle == 0:
        for y in range(h):
            dst[y] = main[base + 1:base + 1 + w]
            if p["applyPDPC"]:
                scale = (flog2(w) + flog2(h) - 2) >> 2
                n = min(3 << scale, w)
                wl = 32 >> ((2 * xs[:n]) >> scale)
                dst[y, :n] = np.clip(dst[y, :n] + ((wl * (side[base + 1 + y] - main[base]) + 32) >> 6), 0, max_val)
    else:
        delta_pos = angle * (1 + m)
        for y in range(h):
            delta_int, delta_fract = delta_pos >> 5, delta_pos & 31
            if abs(angle) & 31:
                if p["interpolationFlag"]:
                    f = [16 - (delta_fract >> 1), 32 - (delta_fract >> 1), 16 + (delta_fract >> 1), delta_fract >> 1]
                else:
                    f = [int(v) for v in cubic_taps()[delta_fract]]
                i0 = base + delta_int
                raw = (f[0] * main[i0:i0 + w] + f[1] * main[i0 + 1:i0 + 1 + w] + f[2] * main[i0 + 2:i0 + 2 + w] + f[3] * main[i0 + 3:i0 + 3 + w] + 32) >> 6
                if probe is not None:
                    probe.append((int(raw.min()), int(raw.max())))
                dst[y] = np.clip(_pel(raw), 0, max_val)
            else:
                dst[y] = main[base + delta_int + 1:base + delta_int + 1 + w]
            if p["applyPDPC"]:
                scale = p["angularScale"]
                n = min(3 << scale, w)
                inv_sum = 256 + np.cumsum(np.full(n, inv))             # invAngleSum += invAngle, per x
                wl = 32 >> ((2 * xs[:n]) >> scale)
                lft = side[base + y + (inv_sum >> 9) + 1]
                dst[y, :n] = _pel(dst[y, :n] + ((wl * (lft - dst[y, :n]) + 32) >> 6))
            delta_pos += angle
    return dst if ver else dst.T.copy()


def predict(top, left, w, h, mode, m, bd, probe=None):
    """predIntraAng: the [h, w] int16 prediction from the unfiltered lines top (2w + 1 + m samples) and left (2h + 1 + m), index 0 = the corner of line m.
    probe: a list that receives (min, max) of the unclipped interpolation sums of every row"""
    top, left = np.asarray(top, np.int64), np.asarray(left, np.int64)
    assert top.size == 2 * w + 1 + m and left.size == 2 * h + 1 + m
    p = params(w, h, mode, m)
    if p["refFilterFlag"]:
        top, left = filter_lines(top, left)
    if mode == PLANAR:
        pred = _planar(top, left, w, h)
    elif mode == DC:
        pred = np.full((h, w), _dc(top, left, w, h, m), np.int64)
    else:
        pred = _angular(p, top, left, w, h, m, (1 << bd) - 1, probe)
    if p["applyPDPC"] and mode in (PLANAR, DC):
        scale = (flog2(w) - 2 + flog2(h) - 2 + 2) >> 2
        for y in range(h):
            wt = 32 >> min(31, (y << 1) >> scale)
            wl = 32 >> np.minimum(31, (np.arange(w) << 1) >> scale)
            val = pred[y]
            pred[y] = _pel(val + ((wl * (left[y + 1] - val) + wt * (top[1:w + 1] - val) + 32) >> 6))
    return pred.astype(np.int16)


# ---- the real xPredIntraPlanar through ctypes (it touches no object state: a dummy `this`) ----------------------------------------------------------------
def ref_planar(top, left, w, h):
    import wp_util
    wp_util.check_layouts()
    fn = ol.ref()._ZN15IntraPrediction16xPredIntraPlanarERK7AreaBufIKsERS0_IsE
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.POINTER(wp_util._AreaBuf), C.POINTER(wp_util._AreaBuf)]
    stride = 2 * w + 1
    src = np.zeros((2, max(stride, 2 * h + 1)), np.int16)   # row 0: top, row 1: left (predStride apart)
    src[0, :stride], src[1, :2 * h + 1] = top, left
    dst = np.zeros((h, w), np.int16)
    s = wp_util._AreaBuf(src.shape[1], 2, src.ctypes.data, src.shape[1])
    d = wp_util._AreaBuf(w, h, dst.ctypes.data, w)
    fn(C.create_string_buffer(64), C.byref(s), C.byref(d))
    return dst


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------------------
def make_lines(rng, w, h, m, bd, kind):
    """kind: 'random', 'alt' (0 and the maximum alternating along each line, the corner shared) or 'const'"""
    nt, nl, mx = 2 * w + 1 + m, 2 * h + 1 + m, (1 << bd) - 1
    if kind == "random":
        top, left = rng.integers(0, mx + 1, nt), rng.integers(0, mx + 1, nl)
    elif kind == "alt":
        ph = int(rng.integers(0, 2))
        top, left = ((np.arange(nt) + ph) & 1) * mx, ((np.arange(nl) + ph) & 1) * mx
    else:
        v = int(rng.integers(0, mx + 1))
        top, left = np.full(nt, v), np.full(nl, v)
    left[0] = top[0]
    return top.astype(np.int16), left.astype(np.int16)


def modes_for(m):
    return list(range(0 if m == 0 else 1, NUM_MODES))


def boundary_modes(w, h):
    """the modes at each rule boundary of a shape: the fixed ones, the first and last mode the wide-angle shift moves, one mode on each side of the MDIS threshold
    (towards HOR and towards VER), an integer-slope and a fractional-slope mode with the filter on"""
    out = {0, 1, 2, 18, 34, 50, 66}
    moved = [k for k in range(2, 67) if wide_angle(w, h, k) != k]
    if moved:
        out |= {moved[0], moved[-1], moved[-1] + 1 if w > h else moved[0] - 1}        # and the first mode the shift leaves alone
    thr = INTRA_FILTER[(flog2(w) + flog2(h)) >> 1]
    for centre in (HOR, VER):
        for d in (thr, thr + 1):
            out |= {k for k in (centre - d, centre + d) if 2 <= k <= 66}
    filt = [k for k in range(2, 67) if params(w, h, k, 0)["refFilterFlag"]]
    frac = [k for k in range(2, 67) if params(w, h, k, 0)["interpolationFlag"]]
    out |= set(filt[:1]) | set(frac[:1]) | set(frac[-1:])
    return sorted(out)


def embed(lines_list, rng=None):
    """the lines of every block between runs of POISON longer than any line: (buffer, refOff per block)"""
    gap = max(max(t.size, l.size) for t, l in lines_list) + 7
    parts, offs, acc = [np.full(gap, POISON, np.int16)], [], gap
    for t, l in lines_list:
        offs.append(acc)
        parts += [t, l, np.full(gap, POISON, np.int16)]
        acc += t.size + l.size + gap
    return np.concatenate(parts), offs


FIRST_ROUND = [0, 1] + list(range(2, 67, 2))    # the 35 modes of the first pre-selection round


def make_block(rng, w, h, m, bd, kind, modes=None):
    top, left = make_lines(rng, w, h, m, bd, kind)
    return dict(w=w, h=h, m=m, bd=bd, top=top, left=left, modes=modes_for(m) if modes is None else list(modes))


def place_in_plane(rng, blocks, stride=97):
    """an original plane with stride > every width and an unaligned position (an odd sample offset) per block: sets org_off / org_stride, returns the int16 plane"""
    rows = sum(b["h"] for b in blocks) + 3
    plane, y = np.zeros((rows, stride), np.int16), 1
    for b in blocks:
        x = int(rng.integers(1, stride - b["w"] - 1))
        x += 1 - ((y * stride + x) & 1)                           # an odd sample offset: no alignment to lean on
        plane[y:y + b["h"], :] = rng.integers(0, 1 << b["bd"], (b["h"], stride))
        b["org_off"], b["org_stride"], b["org_xy"] = y * stride + x, stride, (x, y)
        y += b["h"]
    return plane


class Batch:
    """The tables of a list of blocks (make_block dicts) and their jobs in `order` (default: block after block, mode after mode), the lines embedded between runs
    of POISON.  exp[k]: the restatement's prediction of job k."""

    def __init__(self, blocks, order=None, fill=0xa5):
        from vtm_amd import lib
        self.lib, self.blocks, self.fill = lib, blocks, fill
        self.ref_buf, ref_offs = embed([(b["top"], b["left"]) for b in blocks])
        self.blk_arr = (lib.IntraBlock * len(blocks))()
        jobs, pred_off = [], 0
        for i, b in enumerate(blocks):
            self.blk_arr[i] = lib.IntraBlock(ref_offs[i], b.get("org_off", 0), b.get("org_stride", 0), b["w"], b["h"], b["bd"], b["m"])
            for mode in b["modes"]:
                jobs.append((i, mode, pred_off))
                pred_off += b["w"] * b["h"]
        self.pred_len = pred_off
        self.jobs = [jobs[k] for k in order] if order is not None else jobs
        self.n = len(self.jobs)
        self.job_arr = (lib.IntraJob * max(self.n, 1))(*[lib.IntraJob(off, i, mode) for i, mode, off in self.jobs])
        self._exp, self.probe = None, []      # probe: (min, max) of the unclipped interpolation sums of every row of every job

    @property
    def exp(self):
        if self._exp is None:
            self._exp = [predict(self.blocks[i]["top"], self.blocks[i]["left"], self.blocks[i]["w"], self.blocks[i]["h"], mode, self.blocks[i]["m"],
                                 self.blocks[i]["bd"], self.probe) for i, mode, _ in self.jobs]
        return self._exp

    def _upload(self, ctx):
        from vtm_amd.device import struct_array_to_numpy
        return ctx.to_device(self.ref_buf), ctx.to_device(struct_array_to_numpy(self.blk_arr)), ctx.to_device(struct_array_to_numpy(self.job_arr))

    def run_pred(self, ctx, keep=False):
        """-> the flat int16 prediction buffer (pre-filled with the fill byte), or the device buffers too"""
        d_ref, d_blk, d_job = self._upload(ctx)
        d_pred = ctx.to_device(np.full(max(self.pred_len, 1) * 2, self.fill, np.uint8))
        ctx.intra_pred_batch(d_ref.ptr, d_blk.ptr, len(self.blocks), d_job.ptr, self.n, d_pred.ptr)
        ctx.sync()
        flat = d_pred.to_host(np.int16, shape=(-1,))
        if keep:
            return flat, (d_ref, d_blk, d_job, d_pred)
        for b in (d_ref, d_blk, d_job, d_pred):
            b.free()
        return flat

    def check_pred(self, flat, skip=()):
        for k, (i, mode, off) in enumerate(self.jobs):
            if k in skip:
                continue
            b = self.blocks[i]
            got = flat[off:off + b["w"] * b["h"]].reshape(b["h"], b["w"])
            assert np.array_equal(got, self.exp[k]), (k, b["w"], b["h"], mode, b["m"], b["bd"], np.argwhere(got != self.exp[k])[:4].tolist())

    def run_presel(self, ctx, plane):
        d_ref, d_blk, d_job = self._upload(ctx)
        d_org = ctx.to_device(plane)
        d_out = ctx.to_device(np.full(max(self.n, 1) * 16, self.fill, np.uint8))
        ctx.intra_presel_batch(d_ref.ptr, d_org.ptr, d_blk.ptr, len(self.blocks), d_job.ptr, self.n, d_out.ptr)
        ctx.sync()
        res = d_out.to_host(np.uint64, shape=(-1, 2))
        for b in (d_ref, d_blk, d_job, d_org, d_out):
            b.free()
        return res

    def exp_dist(self, plane):
        """[n, 2] (SAD, SATD) of the restatement's predictions through the oracle's distortions"""
        out = np.zeros((self.n, 2), np.uint64)
        for k, (i, mode, _) in enumerate(self.jobs):
            b = self.blocks[i]
            x, y = b["org_xy"]
            org = ol.i16(plane[y:y + b["h"], x:x + b["w"]])
            out[k] = (ol.o_dist(0, org, ol.i16(self.exp[k]), b["w"], b["h"]), ol.o_dist(1, org, ol.i16(self.exp[k]), b["w"], b["h"]))
        return out
