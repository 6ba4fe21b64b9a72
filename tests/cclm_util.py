"""Numpy restatement of the reference's chroma intra prediction for 4:2:0 without BDPCM (VTM 9.3 CommonLib/IntraPrediction.cpp): the down-sampled luma of
xGetLumaRecPixels :1324-1579, the model parameters of xGetLMParameters :1580-1795, the linear model of predIntraChromaLM :268-288, and the chroma variants of the
regular modes (initPredIntraParams :356-444 with !isLuma, the two-tap branch of xPredIntraAng :592-604).  Written after the reference loop for loop -- three
separate down-sampling loops (top row, left column, inner block) into one buffer with a border, the template walk with startPos / pickStep, the pointer swaps of
the min / max grouping -- and independently of vtm_amd/csrc/cclm_rules.hpp, which has one closed form per down-sampled sample.  Plus the case generators and the
table packing (Batch) the GPU tests and the bench share.

A block is a dict: w, h, bd, above, left (bool), ar, bl (available above-right / below-left chroma samples, before the reference's clamp), first_row, coloc,
lines[c] = (top, left) of Cb and Cr (2w + 1 and 2h + 1 samples, index 0 = the corner), plane (the luma reconstruction, 2-D int16), lxy = (x, y) of the luma
sample co-located with chroma (0, 0), modes."""
import numpy as np

import intra_util as iu

LM, MDLM_L, MDLM_T = 67, 68, 69
NUM_CHROMA_MODES = 70
UNIT = 2                                           # (1 << MIN_CU_LOG2) >> 1: the chroma unit of the availability walk
SIDES = (4, 8, 16, 32)
SHAPES10 = [(4, 4), (8, 4), (4, 8), (8, 8), (16, 4), (4, 16), (16, 16), (32, 8), (8, 32), (32, 32)]
DIV_SIG_TABLE = [0, 7, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 1, 1, 0]     # H.266 8.4.5.2.14 divSigTable
POISON = 0x7fff
AVAIL_CLASSES = ("none", "above", "left", "both", "partial", "full")


def floor_log2(v):
    return -1 if v == 0 else int(v).bit_length() - 1


# ---- xGetLumaRecPixels ------------------------------------------------------------------------------------------------------------------------------------------
def downsample(b, mdlm):
    """-> (inner [h, w], top [w + added above-right] or None, left [h + added below-left] or None); mdlm: the MDLM extents (m_pMdlmTemp) instead of LM's"""
    w, h, plane = b["w"], b["h"], b["plane"].astype(np.int64)
    x0, y0 = b["lxy"]

    def src(x, y):
        return int(plane[y0 + y, x0 + x])

    top = left = None
    if b["above"]:
        n = w + (b["ar"] if mdlm else 0)
        top = np.zeros(n, np.int64)
        for i in range(n):
            pad = i == 0 and not b["left"]
            lx = 2 * i - (0 if pad else 1)
            if b["first_row"]:
                top[i] = (src(2 * i, -1) * 2 + src(lx, -1) + src(2 * i + 1, -1) + 2) >> 2
            elif b["coloc"]:
                top[i] = (4 + src(2 * i, -3) + src(2 * i, -2) * 4 + src(lx, -2) + src(2 * i + 1, -2) + src(2 * i, -1)) >> 3
            else:
                top[i] = (4 + src(2 * i, -2) * 2 + src(2 * i + 1, -2) + src(lx, -2) + src(2 * i, -1) * 2 + src(2 * i + 1, -1) + src(lx, -1)) >> 3
    if b["left"]:
        n = h + (b["bl"] if mdlm else 0)
        left = np.zeros(n, np.int64)
        for j in range(n):
            y = 2 * j                                # piSrc = pRecSrc0 - 1 - logSubWidthC, advancing by two rows
            if b["coloc"]:
                pad = j == 0 and not b["above"]
                left[j] = (4 + src(-2, y - (0 if pad else 1)) + src(-2, y) * 4 + src(-3, y) + src(-1, y) + src(-2, y + 1)) >> 3
            else:
                left[j] = (4 + src(-2, y) * 2 + src(-1, y) + src(-3, y) + src(-2, y + 1) * 2 + src(-1, y + 1) + src(-3, y + 1)) >> 3
    inner = np.zeros((h, w), np.int64)
    for j in range(h):
        for i in range(w):
            lpad, apad = i == 0 and not b["left"], j == 0 and not b["above"]
            lx = 2 * i - (0 if lpad else 1)
            if b["coloc"]:
                inner[j, i] = (4 + src(2 * i, 2 * j - (0 if apad else 1)) + src(2 * i, 2 * j) * 4 + src(lx, 2 * j) + src(2 * i + 1, 2 * j) + src(2 * i, 2 * j + 1)) >> 3
            else:
                inner[j, i] = (4 + src(2 * i, 2 * j) * 2 + src(2 * i + 1, 2 * j) + src(lx, 2 * j) + src(2 * i, 2 * j + 1) * 2 + src(2 * i + 1, 2 * j + 1) +
                               src(lx, 2 * j + 1)) >> 3
    return inner, top, left


# ---- xGetLMParameters -------------------------------------------------------------------------------------------------------------------------------------------
def pairs_to_params(luma, chroma, cnt, bd, info=None):
    """the rule from the selected (luma, chroma) pairs on: -> (a, b, shift); info: a dict that receives which branches were taken"""
    luma, chroma = [int(v) for v in luma] + [0] * 4, [int(v) for v in chroma] + [0] * 4
    luma, chroma = luma[:4], chroma[:4]
    info = {} if info is None else info
    if cnt == 0:
        info["none"] = True
        return 0, 1 << (bd - 1), 0
    if cnt == 2:
        luma[3], chroma[3] = luma[0], chroma[0]
        luma[2], chroma[2] = luma[1], chroma[1]
        luma[0], chroma[0] = luma[1], chroma[1]
        luma[1], chroma[1] = luma[3], chroma[3]
    mn, mx = [0, 2], [1, 3]
    if luma[mn[0]] > luma[mn[1]]:
        mn[0], mn[1] = mn[1], mn[0]
    if luma[mx[0]] > luma[mx[1]]:
        mx[0], mx[1] = mx[1], mx[0]
    if luma[mn[0]] > luma[mx[1]]:
        mn, mx = mx, mn
    if luma[mn[1]] > luma[mx[0]]:
        mn[1], mx[0] = mx[0], mn[1]
    min_l, min_c = (luma[mn[0]] + luma[mn[1]] + 1) >> 1, (chroma[mn[0]] + chroma[mn[1]] + 1) >> 1
    max_l, max_c = (luma[mx[0]] + luma[mx[1]] + 1) >> 1, (chroma[mx[0]] + chroma[mx[1]] + 1) >> 1
    diff = max_l - min_l
    if diff <= 0:
        info["diff0"] = True
        return 0, min_c, 0
    diff_c = max_c - min_c
    x = floor_log2(diff)
    norm = ((diff << 4) >> x) & 15
    v = DIV_SIG_TABLE[norm] | 8
    x += int(norm != 0)
    y = floor_log2(abs(diff_c)) + 1
    add = (1 << y) >> 1
    a = (diff_c * v + add) >> y
    shift = 3 + x - y
    if shift < 1:
        shift = 1
        a = 0 if a == 0 else -15 if a < 0 else 15
        info["clamp"] = a
    info["a"] = a
    return a, min_c - ((a * min_l) >> shift), shift


def template(b, mode, info=None):
    """(use above, use left, top template samples, left template samples) of a mode"""
    w, h = b["w"], b["h"]
    above, left = bool(b["above"]), bool(b["left"])
    n_top = n_left = 0
    if mode == MDLM_T:
        left = False
        ar_units = b["ar"] // UNIT if above else 0
        if ar_units > h // UNIT:
            ar_units = h // UNIT
            if info is not None:
                info["ar_clamp"] = True
        n_top = UNIT * ((w // UNIT if above else 0) + ar_units)
    elif mode == MDLM_L:
        above = False
        bl_units = b["bl"] // UNIT if left else 0
        if bl_units > w // UNIT:
            bl_units = w // UNIT
            if info is not None:
                info["bl_clamp"] = True
        n_left = UNIT * ((h // UNIT if left else 0) + bl_units)
    else:
        n_top, n_left = w, h
    return above, left, n_top, n_left


def lm_params(b, c, mode, ds=None, info=None):
    """(a, b, shift) of component c (0 Cb, 1 Cr) and LM mode 67 / 68 / 69"""
    _, ds_top, ds_left = ds if ds is not None else downsample(b, mode != LM)
    c_top, c_left = b["lines"][c]
    above, left, n_top, n_left = template(b, mode, info)
    above_is4, left_is4 = (0 if left else 1), (0 if above else 1)
    start = [n_top >> (2 + above_is4), n_left >> (2 + left_is4)]
    step = [max(1, n_top >> (1 + above_is4)), max(1, n_left >> (1 + left_is4))]
    sel_l, sel_c, cnt_t, cnt_l = [0] * 4, [0] * 4, 0, 0
    if above:
        cnt_t = min(n_top, (1 + above_is4) << 1)
        pos = start[0]
        for k in range(cnt_t):
            sel_l[k], sel_c[k] = ds_top[pos], c_top[1 + pos]
            pos += step[0]
    if left:
        cnt_l = min(n_left, (1 + left_is4) << 1)
        pos = start[1]
        for k in range(cnt_l):
            sel_l[k + cnt_t], sel_c[k + cnt_t] = ds_left[pos], c_left[1 + pos]
            pos += step[1]
    return pairs_to_params(sel_l, sel_c, cnt_t + cnt_l, b["bd"], info)


# ---- the regular modes of a chroma block ------------------------------------------------------------------------------------------------------------------------
def chroma_params(w, h, mode):
    p = iu.params(w, h, mode, 0)
    p["refFilterFlag"] = p["interpolationFlag"] = 0      # :409: !isLuma( chType )
    return p


def _angular_chroma(p, top, left, w, h, max_val):
    """xPredIntraAng with channelType chroma (multiRefIdx 0): the extended main reference as an array, rows advancing by deltaPos += intraPredAngle"""
    ver, angle, inv = bool(p["isModeVer"]), p["intraPredAngle"], p["invAngle"]
    off = 40
    ref_above, ref_left = np.zeros(off + 2 * 32 + 8, np.int64), np.zeros(off + 2 * 32 + 8, np.int64)
    if angle < 0:
        ref_above[off:off + w + 2] = top[:w + 2]
        ref_left[off:off + h + 2] = left[:h + 2]
        main, side = (ref_above, ref_left) if ver else (ref_left, ref_above)
        size_side = h if ver else w
        for k in range(-size_side, 0):
            main[off + k] = side[off + min((-k * inv + 256) >> 9, size_side)]
    else:
        ref_above[off:off + 2 * w + 1] = top
        ref_left[off:off + 2 * h + 1] = left
        main, side = (ref_above, ref_left) if ver else (ref_left, ref_above)
        ref_length = 2 * w if ver else 2 * h
        main[off + ref_length + 1:off + ref_length + 3] = main[off + ref_length]
    if not ver:
        w, h = h, w
    dst, xs = np.zeros((h, w), np.int64), np.arange(w)
    if angle == 0:
        for y in range(h):
            dst[y] = main[off + 1:off + 1 + w]
            if p["applyPDPC"]:
                scale = (iu.flog2(w) + iu.flog2(h) - 2) >> 2
                n = min(3 << scale, w)
                wl = 32 >> ((2 * xs[:n]) >> scale)
                dst[y, :n] = np.clip(dst[y, :n] + ((wl * (side[off + 1 + y] - main[off]) + 32) >> 6), 0, max_val)
    else:
        delta_pos = angle
        for y in range(h):
            delta_int, delta_fract = delta_pos >> 5, delta_pos & 31
            if abs(angle) & 31:
                p0, p1 = main[off + delta_int + 1:off + delta_int + 1 + w], main[off + delta_int + 2:off + delta_int + 2 + w]
                dst[y] = iu._pel(p0 + ((delta_fract * (p1 - p0) + 16) >> 5))
            else:
                dst[y] = main[off + delta_int + 1:off + delta_int + 1 + w]
            if p["applyPDPC"]:
                scale = p["angularScale"]
                n = min(3 << scale, w)
                inv_sum = 256 + np.cumsum(np.full(n, inv))
                wl = 32 >> ((2 * xs[:n]) >> scale)
                lft = side[off + y + (inv_sum >> 9) + 1]
                dst[y, :n] = iu._pel(dst[y, :n] + ((wl * (lft - dst[y, :n]) + 32) >> 6))
            delta_pos += angle
    return dst if ver else dst.T.copy()


def predict_regular(top, left, w, h, mode, bd):
    """predIntraAng of a chroma block for mode 0 .. 66"""
    top, left = np.asarray(top, np.int64), np.asarray(left, np.int64)
    assert top.size == 2 * w + 1 and left.size == 2 * h + 1
    p = chroma_params(w, h, mode)
    if mode == iu.PLANAR:
        pred = iu._planar(top, left, w, h)
    elif mode == iu.DC:
        pred = np.full((h, w), iu._dc(top, left, w, h, 0), np.int64)
    else:
        pred = _angular_chroma(p, top, left, w, h, (1 << bd) - 1)
    if p["applyPDPC"] and mode in (iu.PLANAR, iu.DC):
        scale = (iu.flog2(w) - 2 + iu.flog2(h) - 2 + 2) >> 2
        for y in range(h):
            wt = 32 >> min(31, (y << 1) >> scale)
            wl = 32 >> np.minimum(31, (np.arange(w) << 1) >> scale)
            val = pred[y]
            pred[y] = iu._pel(val + ((wl * (left[y + 1] - val) + wt * (top[1:w + 1] - val) + 32) >> 6))
    return pred.astype(np.int16)


def predict(b, mode, ds_cache=None):
    """-> [2, h, w] int16: the Cb and Cr predictions of a block for mode 0 .. 69"""
    w, h, bd = b["w"], b["h"], b["bd"]
    if mode < LM:
        return np.stack([predict_regular(b["lines"][c][0], b["lines"][c][1], w, h, mode, bd) for c in (0, 1)])
    ds_cache = {} if ds_cache is None else ds_cache
    mdlm = mode != LM
    if mdlm not in ds_cache:
        ds_cache[mdlm] = downsample(b, mdlm)
    ds, out = ds_cache[mdlm], []
    for c in (0, 1):
        a, off, shift = lm_params(b, c, mode, ds)
        out.append(np.clip(((a * ds[0]) >> shift) + off, 0, (1 << bd) - 1))
    return np.stack(out).astype(np.int16)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------------------
def availability(cls, w, h, k=0):
    """(above, left, ar, bl) of an availability class; 'partial': half the reach (a multiple of the unit), alternating sides"""
    if cls == "none":
        return False, False, 0, 0
    if cls == "above":
        return True, False, (0, w)[k & 1], 0
    if cls == "left":
        return False, True, 0, (0, h)[k & 1]
    if cls == "both":
        return True, True, 0, 0
    if cls == "partial":
        return True, True, max(UNIT, w // 2), max(UNIT, h // 2) if k & 1 else 0
    return True, True, w, h


def make_block(rng, w, h, bd, kind, cls, coloc=False, first_row=False, modes=None, stride=None, k=0, avail=None):
    """kind: 'random', 'alt' (0 / maximum alternating in luma and in the chroma lines), 'const', 'swing' (luma within a few codes of one value, the chroma lines
    alternating: the largest slopes).  The luma plane is POISON wherever the host is not required to supply samples."""
    above, left, ar, bl = availability(cls, w, h, k) if avail is None else avail
    mx = (1 << bd) - 1
    x0 = 4
    need = x0 + 2 * (w + ar) + 1
    stride = need + 2 if stride is None else stride
    assert stride >= need, (stride, need)
    y0 = 3
    rows = y0 + 2 * (h + bl) + 1
    if (y0 * stride + x0) % 2 == 0:
        x0 -= 1                                        # an odd sample offset: no alignment to lean on
    plane = np.full((rows, stride), POISON, np.int16)

    def fill(ya, yb, xa, xb):
        shape = (yb - ya, xb - xa)
        if kind == "random":
            v = rng.integers(0, mx + 1, shape)
        elif kind == "alt":
            v = ((np.add.outer(np.arange(ya, yb), np.arange(xa, xb)) // 2) & 1) * mx
        elif kind == "const":
            v = np.full(shape, fill.c)
        else:
            v = np.clip(fill.c + rng.integers(-2, 3, shape), 0, mx)
        plane[y0 + ya:y0 + yb, x0 + xa:x0 + xb] = v

    fill.c = int(rng.integers(0, mx + 1))
    fill(0, 2 * h, 0, 2 * w)
    if above:
        fill(-3, 0, -3 if left else 0, 2 * (w + ar))
    if left:
        fill(-3 if above else 0, 2 * (h + bl), -3, 0)
    lines = []
    for c in (0, 1):
        t, l = iu.make_lines(rng, w, h, 0, bd, {"swing": "alt"}.get(kind, kind))
        lines.append((t, l))
    return dict(w=w, h=h, bd=bd, above=above, left=left, ar=ar, bl=bl, first_row=bool(first_row and above), coloc=bool(coloc), lines=lines, plane=plane,
                lxy=(x0, y0), modes=list(range(NUM_CHROMA_MODES)) if modes is None else list(modes))


PRESEL_MODES = [1, 18, 50, MDLM_L, MDLM_T]      # estIntraPredChromaQT's pre-selection set: DC, HOR, VER (planar, DM and LM are kept without it) and both MDLM
ALL_LM = [LM, MDLM_L, MDLM_T]


def place_orgs(rng, blocks, stride=97):
    """Cb and Cr original planes (one array, Cb rows first) with an odd sample offset per block: sets org_off = (cb, cr), org_stride, org_xy; returns the plane"""
    rows = sum(b["h"] for b in blocks) + 3
    plane = np.zeros((2 * rows, stride), np.int16)
    y = 1
    for b in blocks:
        x = int(rng.integers(1, stride - b["w"] - 1))
        x += 1 - ((y * stride + x) & 1)
        for c in (0, 1):
            plane[c * rows + y:c * rows + y + b["h"], :] = rng.integers(0, 1 << b["bd"], (b["h"], stride))
        b["org_off"] = (y * stride + x, (rows + y) * stride + x + (1 if (rows * stride) & 1 else 0))
        b["org_stride"], b["org_xy"] = stride, [(x, y), (x + (1 if (rows * stride) & 1 else 0), rows + y)]
        y += b["h"]
    return plane


class Batch:
    """The device tables of a list of blocks and their jobs in `order` (default: block after block, mode after mode).  The chroma lines lie between runs of POISON,
    the luma planes one after the other in one buffer.  exp[k]: the restatement's [2, h, w] prediction of job k."""

    def __init__(self, blocks, order=None, fill=0xa5):
        from vtm_amd import lib
        self.lib, self.blocks, self.fill = lib, blocks, fill
        line_list = [ln for b in blocks for ln in b["lines"]]
        self.ref_buf, ref_offs = iu.embed(line_list)
        planes, luma_offs, acc = [], [], 0
        for i, b in enumerate(blocks):
            luma_offs.append(acc + b["lxy"][1] * b["plane"].shape[1] + b["lxy"][0])
            b["luma_off"], b["luma_stride"], b["ref_off"] = luma_offs[-1], b["plane"].shape[1], (ref_offs[2 * i], ref_offs[2 * i + 1])
            planes.append(b["plane"].reshape(-1))
            acc += b["plane"].size
        self.luma_buf = np.concatenate(planes)
        self.blk_arr = (lib.IntraChromaBlock * len(blocks))()
        jobs, pred_off = [], 0
        for i, b in enumerate(blocks):
            org = b.get("org_off", (0, 0))
            self.blk_arr[i] = lib.IntraChromaBlock(ref_offs[2 * i], ref_offs[2 * i + 1], org[0], org[1], luma_offs[i], b.get("org_stride", 0), b["plane"].shape[1],
                                                   b["w"], b["h"], b["ar"], b["bl"], b["bd"], int(b["above"]), int(b["left"]), int(b["first_row"]), int(b["coloc"]))
            for mode in b["modes"]:
                jobs.append((i, mode, pred_off))
                pred_off += 2 * b["w"] * b["h"]
        self.pred_len = pred_off
        self.jobs = [jobs[k] for k in order] if order is not None else jobs
        self.n = len(self.jobs)
        self.job_arr = (lib.IntraChromaJob * max(self.n, 1))(*[lib.IntraChromaJob(off, off + self.blocks[i]["w"] * self.blocks[i]["h"], i, mode)
                                                               for i, mode, off in self.jobs])
        self._exp = None

    @property
    def exp(self):
        if self._exp is None:
            caches = [dict() for _ in self.blocks]
            self._exp = [predict(self.blocks[i], mode, caches[i]) for i, mode, _ in self.jobs]
        return self._exp

    def _upload(self, ctx):
        from vtm_amd.device import struct_array_to_numpy
        return (ctx.to_device(self.ref_buf), ctx.to_device(self.luma_buf), ctx.to_device(struct_array_to_numpy(self.blk_arr)),
                ctx.to_device(struct_array_to_numpy(self.job_arr)))

    def run_pred(self, ctx, keep=False):
        d_ref, d_luma, d_blk, d_job = self._upload(ctx)
        d_pred = ctx.to_device(np.full(max(self.pred_len, 1) * 2, self.fill, np.uint8))
        ctx.intra_chroma_pred_batch(d_ref.ptr, d_luma.ptr, d_blk.ptr, len(self.blocks), d_job.ptr, self.n, d_pred.ptr)
        ctx.sync()
        flat = d_pred.to_host(np.int16, shape=(-1,))
        if keep:
            return flat, (d_ref, d_luma, d_blk, d_job, d_pred)
        for buf in (d_ref, d_luma, d_blk, d_job, d_pred):
            buf.free()
        return flat

    def check_pred(self, flat, skip=()):
        for k, (i, mode, off) in enumerate(self.jobs):
            if k in skip:
                continue
            b = self.blocks[i]
            got = flat[off:off + 2 * b["w"] * b["h"]].reshape(2, b["h"], b["w"])
            assert np.array_equal(got, self.exp[k]), (k, b["w"], b["h"], mode, b["bd"], b["above"], b["left"], b["ar"], b["bl"], b["first_row"], b["coloc"],
                                                      np.argwhere(got != self.exp[k])[:4].tolist())

    def run_presel(self, ctx, org_plane):
        d_ref, d_luma, d_blk, d_job = self._upload(ctx)
        d_org = ctx.to_device(org_plane)
        d_out = ctx.to_device(np.full(max(self.n, 1) * 32, self.fill, np.uint8))
        ctx.intra_chroma_presel_batch(d_ref.ptr, d_luma.ptr, d_org.ptr, d_blk.ptr, len(self.blocks), d_job.ptr, self.n, d_out.ptr)
        ctx.sync()
        res = d_out.to_host(np.uint64, shape=(-1, 4))
        for buf in (d_ref, d_luma, d_blk, d_job, d_org, d_out):
            buf.free()
        return res


# ---- tests/golden/cclm.npz --------------------------------------------------------------------------------------------------------------------------------------
GOLDEN_PIC, GOLDEN_CTU = (256, 256), 128          # luma picture of the recording rig, CTU size
GOLDEN_REGULAR = [0, 1, 2, 18, 35, 50, 61, 66]    # the regular modes recorded per case (small blocks; larger ones take [::3])
GOLDEN_UNSET = 0x5555                              # down-sampled positions the reference did not fill


def hash_plane(seed, shape, bd, kind):
    """a plane that depends on nothing but its arguments (the golden file stores the seed, not the samples): 'random' by an integer hash of the position, 'alt',
    'const', 'swing' (luma-like: within a few codes of one value)"""
    h, w = shape
    idx = (np.arange(h, dtype=np.uint64)[:, None] * np.uint64(1315423911) + np.arange(w, dtype=np.uint64)[None, :] * np.uint64(2654435761) + np.uint64(seed * 40503 + 17))
    idx ^= idx >> np.uint64(13)
    idx = (idx * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xffffffffffffffff)
    r = (idx >> np.uint64(29)).astype(np.int64)
    mx = (1 << bd) - 1
    if kind == "random":
        return (r & mx).astype(np.int16)
    if kind == "alt":
        return ((((np.arange(h)[:, None] + np.arange(w)[None, :]) // 2 + seed) & 1) * mx).astype(np.int16)
    if kind == "const":
        return np.full(shape, (seed * 37) & mx, np.int16)
    return np.clip(((seed * 53) & mx) + (r % 5) - 2, 0, mx).astype(np.int16)


def golden_planes(seed, bd, kind):
    """(luma, cb, cr) of a golden case; 'swing': a nearly flat luma under alternating chroma"""
    (pw, ph), ckind = GOLDEN_PIC, {"swing": "alt"}.get(kind, kind)
    return hash_plane(seed, (ph, pw), bd, kind), hash_plane(seed + 1, (ph // 2, pw // 2), bd, ckind), hash_plane(seed + 2, (ph // 2, pw // 2), bd, ckind)


def golden_block(hdr, lines):
    """the block dict of a golden case: hdr = (w, h, bd, coloc, above, left, ar, bl, firstRow, kind index, luma x, luma y, seed), lines = the recorded Cb / Cr lines"""
    w, h, bd, coloc, above, left, ar, bl, first_row, kind, x, y, seed = (int(v) for v in hdr)
    luma = golden_planes(seed, bd, ("random", "alt", "const", "swing")[kind])[0]
    nt, nl = 2 * w + 1, 2 * h + 1
    ln = [(lines[c * (nt + nl):c * (nt + nl) + nt], lines[c * (nt + nl) + nt:(c + 1) * (nt + nl)]) for c in (0, 1)]
    return dict(w=w, h=h, bd=bd, above=bool(above), left=bool(left), ar=ar, bl=bl, first_row=bool(first_row), coloc=bool(coloc), lines=ln, plane=luma, lxy=(x, y), modes=[])


def golden_cases(path):
    """yields (block, ds_lm, ds_mdlm, params [3][2][3], pred_lm [3][2][h][w], regular modes, pred_reg [n][2][h][w]) per recorded case; ds_*: (inner, top 2W, left 2H)"""
    g = np.load(path)
    lp = dp = pp = 0
    for hdr, par in zip(g["hdrs"], g["params"]):
        w, h, nm = int(hdr[0]), int(hdr[1]), int(hdr[13])
        nl, nd = 2 * (2 * w + 2 * h + 2), w * h + 2 * w + 2 * h
        b = golden_block(hdr[:13], g["lines"][lp:lp + nl])
        dss = []
        for _ in range(2):
            d = g["ds"][dp:dp + nd]
            dss.append((d[:w * h].reshape(h, w), d[w * h:w * h + 2 * w], d[w * h + 2 * w:]))
            dp += nd
        p_lm = g["preds"][pp:pp + 6 * w * h].reshape(3, 2, h, w)
        pp += 6 * w * h
        p_rg = g["preds"][pp:pp + 2 * nm * w * h].reshape(nm, 2, h, w)
        pp += 2 * nm * w * h
        lp += nl
        modes = GOLDEN_REGULAR if w * h <= 256 else GOLDEN_REGULAR[(int(hdr[12]) - 1000) % 3::3]      # the generator's rotation: the seed is 1000 + its case counter
        yield b, dss[0], dss[1], par.reshape(3, 2, 3), p_lm, modes, p_rg
