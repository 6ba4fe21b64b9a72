"""Job tables and oracle expectations for vtmhip_motion_compensation_batch_dev: the pictures, one job + its expectation (vo_mc_block -> vo_add_avg -> epilogue), the table of
test_gpu_bipred.test_motion_compensation_fused_matches_oracle (legacy_table: the draws of that test, unchanged) and the tables of tests/test_gpu_mc_paths.py (path_table:
blocks that fit a launch hint, in a guarded layout, neighbours of a wave as different as the kernel allows)."""
import ctypes as C
import functools

import numpy as np

import me_util
import oracle_lib as ol
from vtm_amd import synth
from vtm_amd.lib import PredJob

W, H, MARGIN = 416, 240, 64
FILL = np.int16(0xa5a5 - 0x10000)      # what the guarded output buffers hold where no block lies
BCW_WEIGHTS = (-2, 3, 5, 10)           # getBcwWeight of a non-default BcwIdx (0 and 4: the default pair, plain removeHighFreq)
PHASES = ("copy", "bi0", "hor", "ver", "two", "alt")


class Pictures:
    """Two 4:2:0 reference pictures (border-extended) and an original at one bit depth.  Device layout: references [Y ref0 | Y ref1 | U ref0 | U ref1], originals [Y | U]."""

    def __init__(self, bd):
        fr = [[me_util.to_bit_depth(p, bd) for p in f] for f in synth.gen_frames(W, H, 3, chroma=True)]
        (yb0, self.yo, self.ys), (ub0, self.uo, self.us) = synth.extend_plane(fr[0][0], MARGIN), synth.extend_plane(fr[0][1], MARGIN // 2)
        (yb1, _, _), (ub1, _, _) = synth.extend_plane(fr[1][0], MARGIN), synth.extend_plane(fr[1][1], MARGIN // 2)
        self.bd = bd
        self.org_y, self.org_u = np.ascontiguousarray(fr[2][0]), np.ascontiguousarray(fr[2][1])
        self.refs = np.concatenate([yb0, yb1, ub0, ub1])
        self.base = {(0, 0): 0, (0, 1): yb0.size, (1, 0): 2 * yb0.size, (1, 1): 2 * yb0.size + ub0.size}
        self.planes = {(0, 0): yb0, (0, 1): yb1, (1, 0): ub0, (1, 1): ub1}
        self.orgs = np.concatenate([self.org_y.reshape(-1), self.org_u.reshape(-1)])


@functools.lru_cache(maxsize=None)
def pictures(bd):
    return Pictures(bd)


def fill_job(pic, j, cw, ch, cx, cy, chroma, mode, epi, alt, mv, pred_off, out_off, pred_stride, out_stride, bcw=0):
    """Fills PredJob j for the cw x ch block at (cx, cy) of the luma or the U plane (plane units) and returns (pred, out): the oracle's prediction and epilogue output
    as ch x cw arrays; out is None without an epilogue."""
    L = ol.oracle()
    bd = pic.bd
    st, o0 = (pic.us, pic.uo) if chroma else (pic.ys, pic.yo)
    j.orgOff = (pic.org_y.size + cy * (W // 2) + cx) if chroma else (cy * W + cx)
    j.orgStride = W // 2 if chroma else W
    for l in (0, 1):
        j.refOff[l] = pic.base[(chroma, l)] + o0 + cy * st + cx
        j.refStride[l] = st
        j.mv[l][0], j.mv[l][1] = mv[l]
    j.predOff, j.outOff = pred_off, out_off
    j.predStride, j.outStride = pred_stride, out_stride
    j.width, j.height, j.mode, j.epilogue, j.bitDepth, j.useAltHpelIf, j.chroma = cw, ch, mode, epi, bd, alt, chroma
    j.bcwWeight = bcw
    p = [np.zeros((ch, cw), np.int16), np.zeros((ch, cw), np.int16)]
    for l in ((0, 1) if mode == 2 else (mode,)):
        pl = pic.planes[(chroma, l)]
        refp = pl.ctypes.data + 2 * (o0 + cy * st + cx)
        L.vo_mc_block(1 if chroma else 0, C.c_void_p(refp), st, cw, ch, mv[l][0], mv[l][1], int(mode == 2), bd, alt, ol.P(p[l]), cw)
    if mode == 2:
        pred = np.zeros((ch, cw), np.int16)
        L.vo_add_avg(ol.P(p[0]), cw, ol.P(p[1]), cw, ol.P(pred), cw, cw, ch, bd)
    else:
        pred = p[mode]
    ob = (pic.org_u if chroma else pic.org_y)[cy:cy + ch, cx:cx + cw].astype(np.int32)
    if epi == 2 and bcw not in (0, 4):
        out = np.ascontiguousarray(ob.astype(np.int16))
        L.vo_remove_weight_high_freq(ol.P(out), cw, ol.P(pred), cw, cw, ch, bcw)
    else:
        out = (ob - pred).astype(np.int16) if epi == 1 else (2 * ob - pred).astype(np.int16) if epi == 2 else None
    return pred, out


def legacy_table(bd):
    """The job table of test_motion_compensation_fused_matches_oracle: blocks of 4 .. 128 samples a side (no 4x4 luma), packed back to back with predStride = width, every
    call under the hint 128 x 128.  Returns (pictures, jobs, exp_pred, exp_out, meta, samples); exp_out of a job without an epilogue is zero (the buffer's initial value)."""
    pic = pictures(bd)
    rng = np.random.default_rng(91 if bd == 10 else 91 + bd)
    n = 500 if bd == 10 else 250
    jobs = (PredJob * n)()
    exp_pred, exp_out, meta = [], [], []
    pos = 0
    for k in range(n):
        w, h = int(rng.choice([4, 8, 16, 32, 64, 128])), int(rng.choice([4, 8, 16, 32, 64, 128]))
        chroma, mode, epi, alt = int(k % 3 == 1), int(k % 4 if k % 4 < 3 else 2), int(k % 3), int(k % 7 == 0)
        if w == 4 and h == 4 and not chroma:
            w = 8
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4      # (drawn after the size is final: the block stays inside the picture)
        cw, ch, cx, cy = (w // 2, h // 2, x // 2, y // 2) if chroma else (w, h, x, y)
        mv = [[int(rng.integers(-20 * 16, 20 * 16)), int(rng.integers(-20 * 16, 20 * 16))] for _ in range(2)]
        if k % 5 == 0:
            mv[0][0] &= ~15
        if k % 9 == 0:
            mv[1][1] &= ~31
        pred, out = fill_job(pic, jobs[k], cw, ch, cx, cy, chroma, mode, epi, alt, mv, pos, pos, cw, cw)
        exp_pred.append(pred.reshape(-1))
        exp_out.append((np.zeros((ch, cw), np.int16) if out is None else out).reshape(-1))
        meta.append((cw, ch, chroma, mode, epi))
        pos += cw * ch
    return pic, jobs, exp_pred, exp_out, meta, pos


# ---- tables for one launch path -------------------------------------------------------------------------------------------------------
def jobs_per_wave(lanes):
    """Blocks that share a wave when a block gets `lanes` lanes (jobs [k * JPB, (k + 1) * JPB) of the table)."""
    return max(1, 64 // lanes)


def batch_sizes(lanes):
    """The table lengths a path is run at: 1, JPB - 1 (a lone, partly filled wave), and the largest n <= 200 that is no multiple of JPB and whose number of waves leaves a
    remainder of 2 .. 7 over the eight XCDs the launch order is dealt to."""
    jpb = jobs_per_wave(lanes)
    big = next(n for n in range(200, 0, -1) if (jpb == 1 or n % jpb) and -(-n // jpb) % 8 not in (0, 1))
    return sorted({1, jpb - 1, big} - {0})


def shapes_in_hint(hint):
    """(cw, ch, chroma) of the blocks a table under this hint is made of, in plane units: per class (luma / chroma) x (width a multiple of 8 / not) the largest shapes
    that fit the hint, and the smallest chroma block that fits.  No 4x4 luma (no such PU)."""
    hw, hh = hint
    out = []
    for chroma, sides, keep in ((0, (4, 8, 16, 32, 64), 4), (1, (2, 4, 8, 16, 32), 3)):
        fit = [(w, h) for w in sides for h in sides if w <= hw and h <= hh and not (w == 4 and h == 4 and not chroma)]
        for vec in (1, 0):
            cls = sorted((s for s in fit if (s[0] % 8 == 0) == bool(vec)), key=lambda s: (-s[0] * s[1], -s[0]))
            out += [(w, h, chroma) for w, h in cls[:keep]]
        small = min(fit, key=lambda s: (s[0] * s[1], s[0]))
        if chroma and (small[0], small[1], 1) not in out:
            out.append((small[0], small[1], 1))
    return out


def width_class(j):
    """mc_block_vec (eight samples per lane) or mc_block (one)"""
    return "vec" if j.width % 8 == 0 else "scalar"


def phase_class(j):
    """Which way through the block filter a job takes, read from its table entry: the list-0 vector of a bi job, the used list's of a uni job."""
    m = 31 if j.chroma else 15
    fr = [(j.mv[l][0] & m, j.mv[l][1] & m) for l in (0, 1)]
    if j.mode == 2 and fr == [(0, 0), (0, 0)]:
        return "bi0"
    fx, fy = fr[1] if j.mode == 1 else fr[0]
    if j.useAltHpelIf and not j.chroma and (fx or fy) and all(f in (0, 8) for f in (fx, fy)):
        return "alt"
    return "copy" if not (fx or fy) and j.mode != 2 else "hor" if not fy else "ver" if not fx else "two"


class PathTable:
    """n jobs under one hint: jobs (PredJob array), exp_pred / exp_out (the WHOLE output buffers as the call must leave them: FILL outside the blocks and where a job has no
    epilogue), blocks (per job: offsets, strides, size)."""


@functools.lru_cache(maxsize=None)
def path_table(hint, bd, seed, n):
    pic = pictures(bd)
    rng = np.random.default_rng(seed)
    shapes = shapes_in_hint(hint)
    vec, scalar = [s for s in shapes if s[0] % 8 == 0], [s for s in shapes if s[0] % 8]
    t = PathTable()
    t.hint, t.bd, t.n, t.pic = hint, bd, n, pic
    t.jobs = (PredJob * n)()
    blocks, pos_p, pos_o = [], 0, 3
    for k in range(n):
        pool = scalar if (k + k // 4) % 2 and scalar else (vec or scalar)      # neighbours alternate between the two block filters; the pairing shifts every four jobs
        luma = [s for s in pool if not s[2]]
        if luma and (len(luma) == len(pool) or rng.integers(0, 3)):             # two luma blocks for one chroma block, where the filter's pool has both
            pool = luma
        elif luma:
            pool = [s for s in pool if s[2]]
        cw, ch, chroma = pool[int(rng.integers(0, len(pool)))]
        phase = PHASES[k % 6]
        mode = 2 if phase == "bi0" else int(rng.integers(0, 2)) if phase == "copy" else int(rng.integers(0, 3))
        epi = int(rng.integers(0, 3))
        bcw = int(rng.choice((0, 4) + BCW_WEIGHTS)) if epi == 2 else 0
        fb = 5 if chroma else 4
        x, y = int(rng.integers(0, (W - (cw << chroma)) // 4 + 1)) * 4, int(rng.integers(0, (H - (ch << chroma)) // 4 + 1)) * 4
        cx, cy = x >> chroma, y >> chroma
        mv, alt = [], int(phase == "alt" or rng.integers(0, 7) == 0)           # the flag at other fractions than 8 must change nothing
        for l in (0, 1):
            fx, fy = int(rng.integers(1, 1 << fb)), int(rng.integers(1, 1 << fb))
            if l == (mode == 1) or phase == "bi0":                              # the list the class is about (a bi job: list 0; list 1 keeps any fraction)
                if phase in ("copy", "bi0"):
                    fx = fy = 0
                elif phase == "hor":
                    fy = 0
                elif phase == "ver":
                    fx = 0
                elif phase == "alt":
                    fx, fy = [(8, 8), (8, 0), (0, 8)][(k // 6) % 3]             # (a chroma block has no alternative filter: to it this is one more fraction)
            reach = 20 >> chroma                                                # whole samples of the plane: well inside the reference's margin
            mv.append([(int(rng.integers(-reach, reach)) << fb) | fx, (int(rng.integers(-reach, reach)) << fb) | fy])
        ps, os_ = cw + (1, 3, 5)[k % 3], cw + (3, 5, 1)[k % 3]                 # odd pads: rows at every 2-byte alignment
        pos_p += int(rng.integers(0, 2)) + int(rng.integers(0, 3)) * 2          # an odd start for about half the jobs
        pos_o += int(rng.integers(0, 2)) + int(rng.integers(0, 3)) * 2
        if pos_o == pos_p:
            pos_o += 2
        pred, out = fill_job(pic, t.jobs[k], cw, ch, cx, cy, chroma, mode, epi, alt, mv, pos_p, pos_o, ps, os_, bcw)
        blocks.append((pos_p, ps, pos_o, os_, cw, ch, pred, out))
        pos_p += ch * ps + 1
        pos_o += ch * os_ + 1
    t.exp_pred, t.exp_out = np.full(pos_p + 8, FILL, np.int16), np.full(pos_o + 8, FILL, np.int16)
    for pp, ps, po, os_, cw, ch, pred, out in blocks:
        for r in range(ch):
            t.exp_pred[pp + r * ps:pp + r * ps + cw] = pred[r]
            if out is not None:
                t.exp_out[po + r * os_:po + r * os_ + cw] = out[r]
    t.blocks = [b[:6] for b in blocks]
    return t
