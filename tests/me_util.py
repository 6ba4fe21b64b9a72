"""Shared helpers for the motion-search tests: builds the same randomized jobs for the oracle (vo_*), the reference
shim (ref_*) and the HIP kernels."""
import ctypes as C

import numpy as np

import oracle_lib as ol
from vtm_amd import synth
from vtm_amd.lib import TzJob as HipTzJob

PU_W = [8, 16, 32, 64, 128, 4, 16, 8, 32, 64, 12, 24, 48]
PU_H = [8, 16, 32, 64, 128, 8, 4, 16]


class Scene:
    """Two frames of the synthetic clip: `cur` (original) and the border-extended reference plane."""

    def __init__(self, w=416, h=240, hard=True, t_ref=0, t_cur=2, margin=160):
        fr = (synth.gen_frames_hard if hard else synth.gen_frames)(w, h, t_cur + 1)
        self.W, self.H = w, h
        self.cur = np.ascontiguousarray(fr[t_cur])
        self.ref_buf, self.ref_off, self.ref_stride = synth.extend_plane(fr[t_ref], margin)
        self.margin = margin


def motion_lambda(qp, bd):
    """The reference's motion lambda of a slice QP (LambdaFromQpEnable, DepQuant; EncSlice.cpp:699-786, RdCost.cpp:79-84): sqrt( 0.57 * 2^((QP + 6 * (bd - 8) - 12) / 3) *
    2^(0.25 / 3) ).  QP 63: 281 / 1 125 / 4 501 at 8 / 10 / 12 bits; 10-bit QP 32: 31.3."""
    return (0.57 * 2.0 ** ((qp + 6 * (bd - 8) - 12) / 3.0) * 2.0 ** (0.25 / 3.0)) ** 0.5


REAL_QPS = (22, 32, 33, 51, 63)      # 12-bit 128x128: QP 32 / 33 = lambda 125.3 / 140.7, either side of the one-word key's limit (130.03)
EDGE = [6e5, 2e7, 3e9]               # beyond the one-word key for every shape; the last two beyond the 32-bit keys (lambda * 126 >= 2^31)


def real_lambdas(bd):
    return [motion_lambda(q, bd) for q in REAL_QPS]


def key_class(w, h, bd, lam, signed=0):
    """Which arg-min key the integer-search kernels pick for a job (MeJob::narrow / MeJob::tiny): "tiny" = distortion + rate < 2^26 whatever the candidate (one 32-bit
    (cost << 6 | index) key), "narrow" = rate < 2^31 (two-word 32-bit keys), "wide" = the 64-bit arg-min.  Only for coverage floors: never for an expected value."""
    if not (lam >= 0.0 and lam * 126.0 < 2147483648.0):
        return "wide"
    top = 65535.0 if signed else float((1 << bd) - 1)
    return "tiny" if float(w * h) * top + lam * 126.0 < 67108864.0 else "narrow"


def key_classes(jobs, bd):
    out = {"tiny": 0, "narrow": 0, "wide": 0}
    for j in jobs:
        out[key_class(j["w"], j["h"], bd, j["lam"], j.get("signed", 0))] += 1
    return out


def random_tz_jobs(scene, n, seed=5, ranges=(64, 96, 192, 384, 8), allow_ext=True, sizes=None, lams=None):
    """lams: the jobs' motion lambdas are drawn from this list (a generator of its own: independent of the jobs' periodic flags) instead of uniform(1, 40); the other
    fields stay what they are without it."""
    jobs = _random_tz_jobs(scene, n, seed, ranges, allow_ext, sizes)
    return draw_lambdas(jobs, lams, seed) if lams else jobs


def draw_lambdas(jobs, lams, seed):
    pick = np.random.default_rng(seed + 77000).integers(0, len(lams), len(jobs))
    for j, i in zip(jobs, pick):
        j["lam"] = float(lams[int(i)])
    return jobs


def _random_tz_jobs(scene, n, seed, ranges, allow_ext, sizes):
    rng = np.random.default_rng(seed)
    jobs = []
    trial = 0
    while len(jobs) < n:
        trial += 1
        w = int(rng.choice(sizes[0] if sizes else PU_W))
        h = int(rng.choice(sizes[1] if sizes else PU_H))
        if w > scene.W or h > scene.H:
            continue
        x = int(rng.integers(0, (scene.W - w) // 4 + 1)) * 4
        y = int(rng.integers(0, (scene.H - h) // 4 + 1)) * 4
        j = dict(w=w, h=h, x=x, y=y, subShift=1 if (h > 8 and w <= 64) else 0,
                 lam=float(rng.uniform(1, 40)), predHor=int(rng.integers(-64, 64)), predVer=int(rng.integers(-64, 64)),
                 mvHor=int(rng.integers(-40 * 16, 40 * 16)), mvVer=int(rng.integers(-30 * 16, 30 * 16)),
                 searchRange=int(rng.choice(ranges)),
                 ext=int(allow_ext and trial % 5 == 0), fast=int(trial % 11 == 0), firstStop=int(trial % 3 != 0),
                 hasInt=int(trial % 4 == 0), intHor=int(rng.integers(-20, 20)), intVer=int(rng.integers(-20, 20)),
                 extra=[(int(rng.integers(-30 * 16, 30 * 16)), int(rng.integers(-30 * 16, 30 * 16)))
                        for _ in range(int(rng.integers(0, 6)))])
        if trial % 7 == 0:
            j["mvHor"] = j["mvVer"] = 0
        jobs.append(j)
    return jobs


def oracle_ctx(scene, j, org_block):
    c = ol.MeCtx()
    c.org = org_block.ctypes.data
    c.orgStride = org_block.shape[1]
    c.ref = scene.ref_buf.ctypes.data + 2 * (scene.ref_off + j["y"] * scene.ref_stride + j["x"])
    c.refStride = scene.ref_stride
    c.w, c.h, c.subShift, c.bitDepth, c.imvShift = j["w"], j["h"], j["subShift"], getattr(scene, "bd", 10), 0
    c.mv = ol.MvCost(j["lam"], j["predHor"], j["predVer"], 2)
    c.picW, c.picH, c.puX, c.puY, c.ctuSize = scene.W, scene.H, j["x"], j["y"], 128
    return c


def oracle_tz_job(j):
    t = ol.TzJob()
    t.mvHor, t.mvVer, t.searchRange = j["mvHor"], j["mvVer"], j["searchRange"]
    t.extendedSettings, t.fastSettings, t.firstSearchStop = j["ext"], j["fast"], j["firstStop"]
    t.hasIntMv2Nx2NPred, t.intMv2Nx2NPredHor, t.intMv2Nx2NPredVer = j["hasInt"], j["intHor"], j["intVer"]
    t.numExtraStart = len(j["extra"])
    for i, (a, b) in enumerate(j["extra"]):
        t.extraStart[i][0], t.extraStart[i][1] = a, b
    return t


def hip_tz_jobs(scene, jobs, cur_stride):
    arr = (HipTzJob * len(jobs))()
    for k, j in enumerate(jobs):
        t = arr[k]
        t.orgOff = j["y"] * cur_stride + j["x"]
        t.refOff = scene.ref_off + j["y"] * scene.ref_stride + j["x"]
        t.orgStride, t.refStride = cur_stride, scene.ref_stride
        t.puX, t.puY, t.width, t.height = j["x"], j["y"], j["w"], j["h"]
        t.subShift, t.imvShift, t.signedSamples = j["subShift"], 0, j.get("signed", 0)
        t.predHor, t.predVer, t.motionLambda = j["predHor"], j["predVer"], j["lam"]
        t.mvHor, t.mvVer, t.searchRange = j["mvHor"], j["mvVer"], j["searchRange"]
        t.extendedSettings, t.fastSettings, t.firstSearchStop = j["ext"], j["fast"], j["firstStop"]
        t.hasIntMv2Nx2NPred, t.intMv2Nx2NPredHor, t.intMv2Nx2NPredVer = j["hasInt"], j["intHor"], j["intVer"]
        t.numExtraStart = len(j["extra"])
        for i, (a, b) in enumerate(j["extra"]):
            t.extraStart[i][0], t.extraStart[i][1] = a, b
    return arr


def run_oracle_tz(scene, jobs):
    L = ol.oracle()
    out = []
    for j in jobs:
        org = np.ascontiguousarray(scene.cur[j["y"]:j["y"] + j["h"], j["x"]:j["x"] + j["w"]])
        c = oracle_ctx(scene, j, org)
        t = oracle_tz_job(j)
        r = ol.MeResult()
        L.vo_tz_search(C.byref(c), C.byref(t), C.byref(r))
        out.append((r.mvX, r.mvY, r.cost, r.dist, r.nEval))
    return out


# ---- whole xMotionEstimation jobs ---------------------------------------------------------------------------------
AMVR_SHIFT = {0: 2, 1: 4, 2: 6, 3: 3}   # cu.imv -> right shift from internal precision (Mv::m_amvrPrecision)


def _round_amvr(v, imv):
    """Mv::roundTransPrecInternal2Amvr on one component."""
    rs = AMVR_SHIFT[imv]
    o = 1 << (rs - 1)
    return (((v + o - 1) >> rs) if v >= 0 else ((v + o) >> rs)) << rs


def random_mest_jobs(scene, n, seed=17, sizes=None, lams=None, bcws=None):
    """(PU, list, refIdx) jobs of InterSearch::xMotionEstimation: uni / bi, every cu.imv mode, AMVP candidates rounded to the AMVR
    precision as the encoder's AMVP lists are, m_uniMvList entries with duplicates.  lams: motion lambdas drawn from this list instead of uniform(1, 40); bcws: the bi
    rows' CU-level BCW weights cycle over this list (0: the default pair)."""
    jobs = _random_mest_jobs(scene, n, seed, sizes)
    if lams:
        draw_lambdas(jobs, lams, seed)
    if bcws:
        for k, j in enumerate(j for j in jobs if j["bi"]):
            j["bcw"] = int(bcws[k % len(bcws)])
    return jobs


def uniform_mest_rows(jobs, imv=0, bi=None):
    """The jobs as rows of a uniform batch: one AMVR mode (candidates on its grid), optionally all uni / all bi."""
    for j in jobs:
        j["imv"] = imv
        if bi is not None:
            j["bi"] = bi
        j["cands"] = [[_round_amvr(v, imv) for v in c] for c in j["cands"]]
        j["mvPred"] = tuple(j["cands"][j["mvpIdx"]])
    return jobs


def run_oracle_mest(scene, jobs, cfgv):
    """vo_motion_estimation per job: ([result key], [(intX, intY, intDist)])"""
    L = ol.oracle()
    cfg = ol.MestCfg(*cfgv)
    exp, exp_int = [], []
    for j in jobs:
        keep = []
        t = oracle_mest_job(scene, j, keep)
        r = ol.MestResult()
        L.vo_motion_estimation(C.byref(cfg), C.byref(t), C.byref(r))
        exp.append(r.key())
        exp_int.append((r.intX, r.intY, r.intDist))
    return exp, exp_int


def _random_mest_jobs(scene, n, seed, sizes):
    rng = np.random.default_rng(seed)
    jobs = []
    t = 0
    while len(jobs) < n:
        t += 1
        w = int(rng.choice(sizes[0] if sizes else PU_W))
        h = int(rng.choice(sizes[1] if sizes else PU_H))
        if w > scene.W or h > scene.H or (w == 4 and h == 4):
            continue
        x = int(rng.integers(0, (scene.W - w) // 4 + 1)) * 4
        y = int(rng.integers(0, (scene.H - h) // 4 + 1)) * 4
        imv = int(rng.choice([0, 0, 0, 1, 2, 3]))
        cands = [[_round_amvr(int(rng.integers(-24 * 16, 24 * 16)), imv), _round_amvr(int(rng.integers(-16 * 16, 16 * 16)), imv)] for _ in range(2)]
        if t % 9 == 0:
            cands[1] = list(cands[0])
        idx = int(rng.integers(0, 2))
        ncand = 2 if t % 6 else 1
        if ncand == 1:
            idx = 0
        extra = [(int(rng.integers(-30 * 16, 30 * 16)), int(rng.integers(-30 * 16, 30 * 16))) for _ in range(int(rng.integers(0, 7)))]
        if len(extra) > 2 and t % 2:
            extra.append(extra[0])   # duplicates exercise the de-duplication loop
        # bi only for widths a VVC PU can have: the reference's x86 removeHighFreq4 (BufferX86.h:873-892) touches just the first four
        # columns of a row, so for the (non-existent) 12-wide PU its scalar and SIMD builds disagree
        bi = int(t % 3 == 0 and (w & (w - 1)) == 0)
        jobs.append(dict(w=w, h=h, x=x, y=y, bi=bi, imv=imv, mvpIdx=idx, numCand=ncand, cands=cands,
                         mvPred=tuple(cands[idx]), mv=(int(rng.integers(-30, 30)) * 16 + int(rng.integers(0, 16)), int(rng.integers(-20, 20)) * 16 + int(rng.integers(0, 16))),
                         idxBits=(int(rng.integers(1, 3)), int(rng.integers(1, 3))), bits=int(rng.integers(3, 12)),
                         searchRange=int(rng.choice([64, 96, 192, 8])), lam=float(rng.uniform(1, 40)), extra=extra,
                         other_seed=int(rng.integers(0, 1 << 30))))
    return jobs


def other_pred(scene, j):
    """Prediction 'from the other list' for the bi-pred target: the co-located reference block displaced a little plus noise."""
    rng = np.random.default_rng(j["other_seed"])
    dx, dy = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
    m = scene.margin
    plane = scene.ref_buf.reshape(-1, scene.ref_stride)
    blk = plane[m + j["y"] + dy:m + j["y"] + dy + j["h"], m + j["x"] + dx:m + j["x"] + dx + j["w"]].astype(np.int32)
    top = (1 << j.get("bd", getattr(scene, "bd", 10))) - 1
    return np.ascontiguousarray(np.clip(blk + rng.integers(-6, 7, blk.shape), 0, top).astype(np.int16))


def oracle_mest_job(scene, j, keep):
    """ctypes job for vo_motion_estimation / ref_motion_estimation; `keep` collects the arrays the pointers refer to."""
    t = ol.MestJob()
    t.org = scene.cur.ctypes.data + 2 * (j["y"] * scene.W + j["x"])
    t.orgStride = scene.W
    t.ref = scene.ref_buf.ctypes.data + 2 * (scene.ref_off + j["y"] * scene.ref_stride + j["x"])
    t.refStride = scene.ref_stride
    if j["bi"]:
        o = other_pred(scene, j)
        keep.append(o)
        t.otherPred, t.otherStride = o.ctypes.data, j["w"]
    t.w, t.h, t.puX, t.puY, t.picW, t.picH, t.ctuSize, t.bitDepth = j["w"], j["h"], j["x"], j["y"], scene.W, scene.H, 128, getattr(scene, "bd", 10)
    t.bi, t.imv, t.mvpIdx, t.numAmvpCand = j["bi"], j["imv"], j["mvpIdx"], j["numCand"]
    t.mvPredHor, t.mvPredVer = j["mvPred"]
    t.mvHor, t.mvVer = j["mv"]
    for i in range(2):
        t.amvpCand[i][0], t.amvpCand[i][1] = j["cands"][i]
        t.mvpIdxBits[i] = j["idxBits"][i]
    t.bits, t.searchRange, t.motionLambda = j["bits"], j["searchRange"], j["lam"]
    t.numExtraStart = len(j["extra"])
    for i, (a, b) in enumerate(j["extra"]):
        t.extraStart[i][0], t.extraStart[i][1] = a, b
    t.bcwWeight = j.get("bcw", 0)      # bi: the searched list's CU-level BCW weight (0: the default pair)
    t.cachedIntMv = j.get("cached", 0)  # uni: rcMv = the block-vector cache's integer vector, xTZSearch with bFastSettings (InterSearch.cpp:3360-3368, :3434-3441)
    return t


def random_affine_jobs(scene, n, seed=5, sizes=(16, 32, 64, 128), bit_depth=10):
    """Affine ME jobs on a scene: control-point vectors = a small rotation / zoom around a translation, predictors near them.  Jobs of a picture
    at another depth than 10 bits carry it ("bd"): the other list's prediction is clipped to it."""
    rng = np.random.default_rng(seed)
    jobs = []
    while len(jobs) < n:
        w, h = int(rng.choice(sizes)), int(rng.choice(sizes))
        if w > scene.W or h > scene.H:
            continue
        x = int(rng.integers(0, (scene.W - w) // 4 + 1)) * 4
        y = int(rng.integers(0, (scene.H - h) // 4 + 1)) * 4
        six = int(rng.integers(0, 2))
        imv = int(rng.choice([0, 0, 0, 1, 2]))
        tx, ty = int(rng.integers(-12 * 16, 12 * 16)), int(rng.integers(-8 * 16, 8 * 16))
        a, b = int(rng.integers(-40, 41)), int(rng.integers(-40, 41))          # per-block vector differences (1/16 sample)
        mv = [[tx, ty], [tx + a, ty + b], [tx - b + int(rng.integers(-8, 9)) * six, ty + a + int(rng.integers(-8, 9)) * six]]
        if len(jobs) % 7 == 0:
            mv = [[tx, ty], [tx, ty], [tx, ty]]        # pure translation: PROF is off, the gradient iteration starts from a flat model
        if len(jobs) % 11 == 0:
            mv[1] = [tx + 900, ty - 700]              # a spread the sub-block vectors may not have (isSubblockVectorSpreadOverLimit)
        pred = [[v[0] + int(rng.integers(-3, 4)) * 4, v[1] + int(rng.integers(-3, 4)) * 4] for v in mv]
        sh = {0: 2, 1: 0, 2: 4}[imv]
        rnd = lambda v: (((v + (1 << sh >> 1) - (1 if v >= 0 else 0)) >> sh) << sh) if sh else v   # noqa: E731
        pred = [[rnd(p[0]), rnd(p[1])] for p in pred]
        jobs.append(dict(w=w, h=h, x=x, y=y, six=six, imv=imv, mv=mv, pred=pred, bi=int(rng.integers(0, 3) == 0), satd=int(rng.integers(0, 4) != 0),
                         affine_type=int(rng.integers(0, 5) != 0), enc_opt=int(imv != 2 and rng.integers(0, 2)), low_delay=int(rng.integers(0, 2)),
                         inter_dir=int(rng.choice([1, 2, 3])), prof=int(rng.integers(0, 4) != 0), prof_large=int(rng.integers(0, 2)), prof_bi=int(rng.integers(0, 2)),
                         bits=int(rng.integers(4, 14)), lam=float(rng.uniform(2, 30)), hevc_scale=float(rng.choice([0.5, 1.0, 4.0])),
                         other_seed=int(rng.integers(0, 1 << 30))))
        if bit_depth != 10:
            jobs[-1]["bd"] = bit_depth
    return jobs


def affine_pred_struct(scene, j, bit_depth=10):
    p = ol.AffinePred()
    p.ref = scene.ref_buf.ctypes.data + 2 * (scene.ref_off + j["y"] * scene.ref_stride + j["x"])
    p.refStride, p.w, p.h, p.puX, p.puY, p.picW, p.picH, p.ctuSize, p.bitDepth = scene.ref_stride, j["w"], j["h"], j["x"], j["y"], scene.W, scene.H, 128, bit_depth
    p.sixParam, p.interDir, p.profAllowed, p.profNeedsLargeGrad, p.profIsBi = j["six"], j["inter_dir"], j["prof"], j["prof_large"], j["prof_bi"]
    return p


def affine_me_struct(scene, j, keep, bit_depth=10):
    t = ol.AffineMeJob()
    t.pred = affine_pred_struct(scene, j, bit_depth)
    t.org, t.orgStride = scene.cur.ctypes.data + 2 * (j["y"] * scene.W + j["x"]), scene.W
    if j["bi"]:
        o = other_pred(scene, j)
        keep.append(o)
        t.otherPred, t.otherStride = o.ctypes.data, j["w"]
    t.bi, t.imv, t.useSatd, t.useAffineType, t.amvrEncOpt, t.lowDelayRounds = j["bi"], j["imv"], j["satd"], j["affine_type"], j["enc_opt"], j["low_delay"]
    for i in range(3):
        t.mvPred[i][0], t.mvPred[i][1] = j["pred"][i]
        t.mv[i][0], t.mv[i][1] = j["mv"][i]
    t.bits, t.motionLambda = j["bits"], j["lam"]
    return t


def to_bit_depth(f, bd):
    """A 10-bit picture of the generator at `bd` bits.  Below 10 bits the low bits go; above, the top bits are repeated into the new low ones and the
    result is stretched by 5/4 about mid-grey and clipped, so that bright and dark areas sit at exactly 0 and 2^bd - 1 and edges span the whole range."""
    f = f.astype(np.int32)
    if bd <= 10:
        return np.ascontiguousarray((f >> (10 - bd)).astype(np.int16))
    v = (f << (bd - 10)) | (f >> (20 - bd))
    mid = 1 << (bd - 1)
    return np.ascontiguousarray(np.clip((v - mid) * 5 // 4 + mid, 0, (1 << bd) - 1).astype(np.int16))


class DeepScene(Scene):
    """`Scene` at another sample depth (to_bit_depth of the same two frames)."""

    def __init__(self, w=416, h=240, hard=True, bit_depth=10, margin=160):
        fr = (synth.gen_frames_hard if hard else synth.gen_frames)(w, h, 3)
        self.bd = bit_depth
        self.W, self.H = w, h
        self.cur = to_bit_depth(fr[2], bit_depth)
        self.ref_buf, self.ref_off, self.ref_stride = synth.extend_plane(to_bit_depth(fr[0], bit_depth), margin)
        self.margin = margin


def make_signed(scene, seed=17, span=None):
    """Turns the scene's original into a bi-pred search target 2*org - other with `other` in 0 .. span - 1 (default: the whole range of the depth): -(2^bd - 1) .. 2 * (2^bd - 1)"""
    bd = getattr(scene, "bd", 10)
    other = np.random.default_rng(seed).integers(0, span or (1 << bd), scene.cur.shape)
    scene.cur = np.ascontiguousarray((2 * scene.cur.astype(np.int32) - other).astype(np.int16))
    scene.signed = 1
    return scene


class SaturatedScene(Scene):
    """A picture pair whose block SADs sit at about w * h * (2^bd - 1) -- what natural pictures never reach: original = bright field (max - noise 0..3) with dark 8x8
    specks (0 .. 63), reference = dark field (noise 0..3) with bright specks (max - 0 .. 63), w * h / 512 specks per plane, so that candidates still differ.  signed: the
    original becomes 2*org - other with other in 0..7: the full positive excursion of a bi-pred target of the depth."""

    def __init__(self, w=416, h=240, bit_depth=10, seed=1, signed=False, margin=160):
        rng = np.random.default_rng(seed)
        top = (1 << bit_depth) - 1
        cur = top - rng.integers(0, 4, (h, w))
        ref = rng.integers(0, 4, (h, w))
        for plane, bright in ((cur, False), (ref, True)):
            for _ in range(w * h // 512):
                x, y = int(rng.integers(0, w - 7)), int(rng.integers(0, h - 7))
                a = rng.integers(0, 64, (8, 8))
                plane[y:y + 8, x:x + 8] = top - a if bright else a
        self.bd, self.W, self.H, self.margin = bit_depth, w, h, margin
        self.cur = np.ascontiguousarray(cur.astype(np.int16))
        self.ref_buf, self.ref_off, self.ref_stride = synth.extend_plane(np.ascontiguousarray(ref.astype(np.int16)), margin)
        if signed:
            make_signed(self, seed + 1, span=8)


BIG = ([128, 128, 64], [128, 128, 64])      # random_*_jobs sizes: 128x128 / 128x64 / 64x128 (and 64x64): the shapes whose distortion alone approaches 2^26 at 12 bits


def near_key_limit(jobs, exp_cost, exp_dist, bd, signed):
    """Floors of a 12-bit saturated-scene test, from the expected results alone: unsigned, the jobs classed "tiny" that end with 2^25 <= cost < 2^26 (the one-word key
    within a factor of two of its limit); signed, the jobs whose distortion alone is >= 2^26."""
    if signed:
        return sum(1 for d in exp_dist if d >= 1 << 26)
    return sum(1 for j, c in zip(jobs, exp_cost) if key_class(j["w"], j["h"], bd, j["lam"], 0) == "tiny" and (1 << 25) <= c < (1 << 26))


def simd_had4_split(j, cfgv, bd):
    """The one class of xMotionEstimation jobs left out of the saturated-scene comparisons against the REAL member: bi rows of width 4 under the BCW weight -2 with the
    Hadamard cost at bitDepth <= 10.  Their target -4 * org + 5 * pred differs from the reference block by up to 5 * (2^bd - 1), and the reference's x86 4x4 / 4x8 / 4x16
    Hadamards for bitDepth <= 10 (16-bit lanes) leave their range there: its scalar xCalcHADs4x4 -- which the oracle equals on every such block -- and its SIMD build return
    different sums (tests/test_oracle_vs_ref.py::test_width4_hadamard_of_a_weight_m2_target_scalar_is_the_arbiter).  Natural scenes never reach it; nothing wider is left out."""
    return bool(j["bi"] and j["w"] == 4 and j.get("bcw", 0) == -2 and cfgv[1] and bd <= 10)


# ---- SMVD (symmetric MVD search of predInterSearch) -------------------------------------------------------------------------------
class SmvdScene(Scene):
    """The original picture between two references: list 0 = an earlier frame (ref_buf), list 1 = a later one (ref_buf2)."""

    def __init__(self, w=416, h=240, hard=False, margin=160, bit_depth=10):
        fr = (synth.gen_frames_hard if hard else synth.gen_frames)(w, h, 5)
        if bit_depth != 10:      # the generator makes 10-bit samples
            fr = [(f.astype(np.int32) << (bit_depth - 10)).astype(np.int16) if bit_depth > 10 else (f >> (10 - bit_depth)).astype(np.int16) for f in fr]
        self.bd = bit_depth
        self.W, self.H = w, h
        self.cur = np.ascontiguousarray(fr[2])
        self.ref_buf, self.ref_off, self.ref_stride = synth.extend_plane(fr[0], margin)
        self.ref_buf2, _, _ = synth.extend_plane(fr[4], margin)
        self.margin = margin


SMVD_SIZES = [(8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (16, 8), (8, 16), (32, 16), (16, 32), (64, 32), (32, 8), (8, 32), (16, 4), (4, 16), (64, 16), (4, 32), (128, 64)]


def random_smvd_jobs(scene, n, seed=3, sizes=None):
    """(PU, AMVP lists, start vectors) as predInterSearch hands them to the SMVD block; vectors in 1/16 sample, candidates at the AMVR precision."""
    rng = np.random.default_rng(seed)
    jobs = []
    while len(jobs) < n:
        w, h = (sizes or SMVD_SIZES)[int(rng.integers(0, len(sizes or SMVD_SIZES)))]
        if w > scene.W or h > scene.H:
            continue
        x = int(rng.integers(0, (scene.W - w) // 4 + 1)) * 4
        y = int(rng.integers(0, (scene.H - h) // 4 + 1)) * 4
        imv = int(rng.choice([0, 0, 0, 1, 2, 3]))
        base = (int(rng.integers(-10 * 16, 10 * 16)), int(rng.integers(-6 * 16, 6 * 16)))
        near = lambda c, r: (_round_amvr(c[0] + int(rng.integers(-r, r + 1)), imv), _round_amvr(c[1] + int(rng.integers(-r, r + 1)), imv))   # noqa: E731
        cands = [[near(base, 40), near(base, 40)], [near((-base[0], -base[1]), 40), near((-base[0], -base[1]), 40)]]
        for l in range(2):
            if rng.integers(0, 6) == 0:
                cands[l][1] = cands[l][0]              # equal candidates: the SMVD block shortens the list (:2668-2671)
        num = [int(rng.choice([1, 2, 2, 2])), int(rng.choice([1, 2, 2, 2]))]
        starts = [near(base, 60) if rng.integers(0, 4) else cands[0][int(rng.integers(0, 2))] for _ in range(int(rng.integers(2, 9)))]
        starts = [(s[0] + int(rng.integers(-2, 3)) * (k >= 3), s[1]) for k, s in enumerate(starts)]   # history entries need not sit on the AMVR grid
        jobs.append(dict(w=w, h=h, x=x, y=y, imv=imv, satd=int(rng.integers(0, 5) != 0), clip=int(rng.integers(0, 3) == 0),
                         bcw=int(rng.choice([4, 4, 4, 4, -2, 3, 5, 10])), num=num, cands=cands, idxBits=[int(rng.integers(1, 3)), int(rng.integers(1, 4))],
                         lam=float(rng.uniform(2, 40)), starts=starts, numFixed=int(rng.integers(2, 4)), modeBits=int(rng.integers(3, 9))))
    return jobs


def smvd_struct(scene, j):
    t = ol.SmvdJob()
    t.org, t.orgStride = scene.cur.ctypes.data + 2 * (j["y"] * scene.W + j["x"]), scene.W
    t.ref[0] = scene.ref_buf.ctypes.data + 2 * (scene.ref_off + j["y"] * scene.ref_stride + j["x"])
    t.ref[1] = scene.ref_buf2.ctypes.data + 2 * (scene.ref_off + j["y"] * scene.ref_stride + j["x"])
    t.refStride[0] = t.refStride[1] = scene.ref_stride
    t.w, t.h, t.puX, t.puY, t.picW, t.picH, t.ctuSize, t.bitDepth = j["w"], j["h"], j["x"], j["y"], scene.W, scene.H, 128, getattr(scene, "bd", 10)
    t.imv, t.useSatd, t.clipBiPred, t.bcwWeightTar = j["imv"], j["satd"], j["clip"], j["bcw"]
    for l in range(2):
        t.numCand[l] = j["num"][l]
        for i in range(2):
            t.cand[l][i][0], t.cand[l][i][1] = j["cands"][l][i]
        t.mvpIdxBits[l] = j["idxBits"][l]
    t.motionLambda = j["lam"]
    return t


def smvd_member_results(scene, j, lib, prefix):
    """(xGetSymmetricCost, xSymmetricMotionEstimation, symmvdCheckBestMvp) results of one job through `lib` (prefix "vo_": oracle, "ref_": the real members).
    Inputs derived from the job alone: start vector starts[0], its mirror around the first predictor pair, costs a little above the start cost."""
    I2 = C.c_int * 2
    t = smvd_struct(scene, j)
    pc, pt, start = j["cands"][0][0], j["cands"][1][0], j["starts"][0]
    pair = (pt[0] - (start[0] - pc[0]), pt[1] - (start[1] - pc[1]))
    fn = getattr(lib, prefix + "symmetric_cost")
    fn.restype = C.c_uint64
    c0 = fn(C.byref(t), I2(*start), I2(*pair))
    mc, mt, cost = I2(*start), I2(*pair), C.c_uint64(c0 + int(j["lam"] * 6))
    getattr(lib, prefix + "symmetric_me")(C.byref(t), I2(*pc), I2(*pt), mc, mt, C.byref(cost))
    me = (tuple(mc), tuple(mt), cost.value)
    pred, idx, cost = (I2 * 2)(I2(*pc), I2(*pt)), I2(0, 0), C.c_uint64(c0 + int(j["lam"] * 9))
    getattr(lib, prefix + "symmvd_check_best_mvp")(C.byref(t), I2(*start), j["x"] // 4 & 1, pred, idx, C.byref(cost))
    return c0, me, (tuple(pred[0]), tuple(pred[1]), tuple(idx), cost.value)


def smvd_search_oracle(scene, j, L):
    t = smvd_struct(scene, j)
    st = ((C.c_int * 2) * len(j["starts"]))(*[(C.c_int * 2)(*v) for v in j["starts"]])
    r = ol.SmvdResult()
    L.vo_smvd_search(C.byref(t), j["numFixed"], len(j["starts"]), st, j["modeBits"], C.byref(r))
    return r.key()


# ---- SMVD job sets of tests/test_gpu_smvd_forms.py (random_smvd_jobs above and its job sets stay what they are) -----------------------------------------------
SMVD_MAX_START = 18      # VTMHIP_SMVD_MAX_START
SMVD_TILE_SHAPES = [(8, 8), (16, 8), (8, 16), (16, 16), (32, 8), (8, 32), (32, 16), (16, 32), (32, 32), (64, 16), (16, 64), (64, 32), (32, 64), (64, 64), (128, 64),
                    (64, 128), (128, 128)]      # the switch of vtmhip_smvd_batch_dev


def smvd_search_oracle_at(scene, j, L, grow=0, max_start=SMVD_MAX_START):
    """smvd_search_oracle with picW, picH and ctuSize each `grow` larger (the limits of clipMv move by that many samples) and the start list cut at `max_start`
    entries (the device takes VTMHIP_SMVD_MAX_START)."""
    t = smvd_struct(scene, j)
    t.picW, t.picH, t.ctuSize = t.picW + grow, t.picH + grow, t.ctuSize + grow
    starts = j["starts"][:max_start]
    st = ((C.c_int * 2) * len(starts))(*[(C.c_int * 2)(*v) for v in starts])
    r = ol.SmvdResult()
    L.vo_smvd_search(C.byref(t), j["numFixed"], len(starts), st, j["modeBits"], C.byref(r))
    return r.key()


def bulk_smvd_jobs(scene, n, seed, size):
    """n jobs of one shape with the fields and ranges of random_smvd_jobs, drawn as arrays (tens of thousands of jobs in well under a second)."""
    rng = np.random.default_rng(seed)
    w, h = size
    ri = lambda lo, hi, *shape: rng.integers(lo, hi, (n,) + shape)   # noqa: E731
    x, y = ri(0, (scene.W - w) // 4 + 1) * 4, ri(0, (scene.H - h) // 4 + 1) * 4
    imv = np.array([0, 0, 0, 1, 2, 3])[ri(0, 6)]
    rs = np.array([AMVR_SHIFT[i] for i in range(4)])[imv]

    def rnd(v):      # _round_amvr on arrays whose last axis is (hor, ver)
        s, o = rs.reshape((n,) + (1,) * (v.ndim - 1)), (1 << (rs - 1)).reshape((n,) + (1,) * (v.ndim - 1))
        return np.where(v >= 0, (v + o - 1) >> s, (v + o) >> s) << s
    base = np.stack([ri(-160, 160), ri(-96, 96)], axis=-1)
    sign = np.array([1, -1]).reshape(1, 2, 1, 1)
    cands = rnd(base.reshape(n, 1, 1, 2) * sign + ri(-40, 41, 2, 2, 2))                 # [job][list][i][hor / ver]
    same = ri(0, 6, 2) == 0
    cands[:, :, 1, :] = np.where(same[:, :, None], cands[:, :, 0, :], cands[:, :, 1, :])   # equal candidates: the SMVD block shortens the list
    num = np.array([1, 2, 2, 2])[ri(0, 4, 2)]
    nstart = ri(2, 9)
    starts = rnd(base.reshape(n, 1, 2) + ri(-60, 61, 8, 2))
    pick = ri(0, 2, 8)
    from_cand = ri(0, 4, 8) == 0
    starts = np.where(from_cand[:, :, None], np.take_along_axis(cands[:, 0], pick[:, :, None], axis=1), starts)
    starts[:, 3:, 0] += ri(-2, 3, 5)                                                     # history entries need not sit on the AMVR grid
    satd, clip, bcw = ri(0, 5) != 0, ri(0, 3) == 0, np.array([4, 4, 4, 4, -2, 3, 5, 10])[ri(0, 8)]
    ib0, ib1, lam, nfix, mode = ri(1, 3), ri(1, 4), rng.uniform(2, 40, n), ri(2, 4), ri(3, 9)
    cl, sl = cands.tolist(), starts.tolist()
    return [dict(w=w, h=h, x=int(x[k]), y=int(y[k]), imv=int(imv[k]), satd=int(satd[k]), clip=int(clip[k]), bcw=int(bcw[k]), num=[int(num[k, 0]), int(num[k, 1])],
                 cands=[[tuple(c) for c in l] for l in cl[k]], idxBits=[int(ib0[k]), int(ib1[k])], lam=float(lam[k]),
                 starts=[tuple(s) for s in sl[k][:int(nstart[k])]], numFixed=int(nfix[k]), modeBits=int(mode[k])) for k in range(n)]


class SmvdNoiseMarginScene(SmvdScene):
    """The hard scene with both reference planes' margins filled with seeded noise (the picture area unchanged): a block read at a clipped vector lies in the margin,
    and under edge replication a clipped and an unclipped block would read the same samples."""

    def __init__(self, w=416, h=240, margin=160, bit_depth=10, seed=4100):
        super().__init__(w, h, hard=True, margin=margin, bit_depth=bit_depth)
        rng = np.random.default_rng(seed)
        for buf in (self.ref_buf, self.ref_buf2):
            v = buf.reshape(-1, self.ref_stride)
            inside = v[margin:margin + h, margin:margin + w].copy()
            v[:] = rng.integers(0, 1 << bit_depth, v.shape).astype(np.int16)
            v[margin:margin + h, margin:margin + w] = inside


def smvd_clip_limits(scene, j):
    """((horMin, horMax), (verMin, verMax)) of clipMv (MVR_CLIP_MIN / MVR_CLIP_MAX, 1/16 sample) for the job's PU"""
    return (((-128 - 8 - j["x"] + 1) << 4, (scene.W + 8 - j["x"] - 1) << 4), ((-128 - 8 - j["y"] + 1) << 4, (scene.H + 8 - j["y"] - 1) << 4))


def clip_smvd_jobs(scene, size, n=48, seed=4200):
    """PUs at the four picture corners (job k: corner k & 3).  In one list -- list (k >> 2) & 1 -- every AMVP candidate (for list 0 every start vector too) lies between 6
    samples inside and 14 samples beyond the clipMv limit the corner faces, in both components for the jobs with (k >> 3) & 1 == 0 and horizontally only for the others;
    the other list points into the picture (with list 1 at the limit the start vectors stay within 3 samples of the first list-0 candidate, so that the mirrored vectors
    stay at the limit).  All vectors on the AMVR grid.  Returns (jobs, zones): zones[k] = (list, ((lo, hi) hor, (lo, hi) ver or None))."""
    rng = np.random.default_rng(seed + size[0] * 131 + size[1])
    w, h = size
    jobs, zones = [], []
    for k in range(n):
        right, bottom, lst, both = k & 1, (k >> 1) & 1, (k >> 2) & 1, not (k >> 3) & 1
        j = dict(w=w, h=h, x=(scene.W - w) * right, y=(scene.H - h) * bottom, imv=int(rng.choice([0, 0, 0, 1, 2, 3])))
        step = 1 << AMVR_SHIFT[j["imv"]]
        lim = smvd_clip_limits(scene, j)
        zone = []
        for c, far in ((0, right), (1, bottom)):
            b = lim[c][far]
            zone.append((b - 6 * 16, b + 14 * 16) if far else (b - 14 * 16, b + 6 * 16))
        if not both:
            zone[1] = None

        def grid(lo, hi):
            return int(rng.integers(-(-lo // step), hi // step + 1)) * step

        def inward(far, lo, hi):      # lo .. hi sixteenths into the picture
            return -grid(lo, hi) if far else grid(lo, hi)

        def at_limit():
            return (grid(*zone[0]), grid(*zone[1]) if both else inward(bottom, 0, 48))

        def inside():
            return (inward(right, 16, 160), inward(bottom, 16, 96))
        cands = [[at_limit(), at_limit()], [inside(), inside()]] if lst == 0 else [[inside(), inside()], [at_limit(), at_limit()]]
        if lst == 0:
            starts = [at_limit() for _ in range(int(rng.integers(3, 9)))]
        else:
            starts = [(cands[0][0][0] + grid(-48, 48), cands[0][0][1] + grid(-48, 48)) for _ in range(int(rng.integers(3, 9)))]
        j.update(satd=int(rng.integers(0, 5) != 0), clip=int(rng.integers(0, 3) == 0), bcw=int(rng.choice([4, 4, 4, 4, -2, 3, 5, 10])), num=[2, 2], cands=cands,
                 idxBits=[int(rng.integers(1, 3)), int(rng.integers(1, 4))], lam=float(rng.uniform(2, 40)), starts=starts, numFixed=int(rng.integers(2, 4)),
                 modeBits=int(rng.integers(3, 9)))
        jobs.append(j)
        zones.append((lst, tuple(zone)))
    return jobs, zones


def smvd_evaluated_starts(j, max_start=SMVD_MAX_START):
    """raw indices of the start entries the SMVD block evaluates (smmvdCandsGen, :2709-2763): the distinct ones in list order -- entries from numFixed on rounded to
    the AMVR precision and taken while fewer than 5 are collected -- that are not one of list 0's (shortened) predictors"""
    c0 = j["cands"][0][:1 if j["num"][0] < 2 or j["cands"][0][0] == j["cands"][0][1] else 2]
    seen, out = [], []
    for s, v in enumerate(j["starts"][:max_start]):
        if s >= j["numFixed"]:
            if len(seen) >= 5:
                break
            if j["imv"]:
                v = (_round_amvr(v[0], j["imv"]), _round_amvr(v[1], j["imv"]))
        v = tuple(v)
        if v in seen:
            continue
        seen.append(v)
        if v not in [tuple(c) for c in c0]:
            out.append(s)
    return out


def long_start_smvd_jobs(scene, n, seed, size, base=None):
    """Jobs with VTMHIP_SMVD_MAX_START start entries: the numFixed fixed ones, then 6 .. 10 entries that equal a fixed one after the AMVR rounding (dropped as
    duplicates), then distinct vectors within +-90 sixteenths of the first list-0 candidate.  A job in four carries numStart = 19 .. 22 (the device clamps it, the
    oracle gets the 18).  base: jobs whose other fields are kept (default: bulk_smvd_jobs)."""
    rng = np.random.default_rng(seed + 17)
    jobs = [dict(j) for j in (base if base is not None else bulk_smvd_jobs(scene, n, seed, size))]
    for k, j in enumerate(jobs):
        imv, step = j["imv"], 1 << AMVR_SHIFT[j["imv"]]
        fixed = [(_round_amvr(s[0], imv), _round_amvr(s[1], imv)) for s in (j["starts"] + j["starts"])[:j["numFixed"]]]      # on the grid: a rounded entry can equal them
        slack = step // 4 if imv else 0
        dups = []
        for _ in range(int(rng.integers(6, 11))):
            f = fixed[int(rng.integers(0, len(fixed)))]
            dups.append((f[0] + int(rng.integers(-slack, slack + 1)), f[1] + int(rng.integers(-slack, slack + 1))))
        c = j["cands"][0][0]
        tail = []      # distinct as listed; the first one also after the rounding, from the fixed entries and list 0's predictors: it is evaluated
        while len(fixed) + len(dups) + len(tail) < SMVD_MAX_START:
            v = (c[0] + int(rng.integers(-90, 91)), c[1] + int(rng.integers(-90, 91)))
            r = (_round_amvr(v[0], imv), _round_amvr(v[1], imv)) if imv else v
            if v not in tail and (tail or r not in fixed + [tuple(p) for p in j["cands"][0]]):
                tail.append(v)
        j["starts"] = fixed + dups + tail
        if k % 4 == 0:
            j["numStart"] = SMVD_MAX_START + 1 + k // 4 % 4
    return jobs


class SmvdFlatScene(SmvdScene):
    """Original and both reference planes constant (three different values): every candidate of a search has the same distortion, so its choices are the
    first-minimum rules alone."""

    def __init__(self, w=416, h=240, margin=160, bit_depth=10):
        super().__init__(w, h, hard=False, margin=margin, bit_depth=bit_depth)
        top = 1 << bit_depth
        self.cur[:], self.ref_buf[:], self.ref_buf2[:] = top // 2, top // 2 - top // 32, top // 2 + top // 16


def _eg_bits(v):
    """bits of one vector-difference component (RdCost::xGetExpGolombNumberOfBits)"""
    t = ((-v) << 1) + 1 if v <= 0 else v << 1
    n = 1
    while t > 128:
        n, t = n + 14, t >> 7
    return n + 2 * (t.bit_length() - 1)


def smvd_tie_counts(scene, j, L):
    """(predictor pairs of least cost, (start entry, pair) candidates of least cost) of a job: xGetSymmetricCost of every predictor pair, and for every evaluated
    start entry and pair the distortion plus the rate rule floor(lambda * (vector bits at the AMVR precision + the two index bits))"""
    t = smvd_struct(scene, j)
    I2 = C.c_int * 2
    cost = lambda a, b: L.vo_symmetric_cost(C.byref(t), I2(*a), I2(*b))      # noqa: E731
    n = [1 if j["num"][l] < 2 or j["cands"][l][0] == j["cands"][l][1] else 2 for l in range(2)]
    pairs = [(i, k) for i in range(n[0]) for k in range(n[1])]
    pc = [cost(j["cands"][0][i], j["cands"][1][k]) for i, k in pairs]
    rs = AMVR_SHIFT[j["imv"]]
    down = lambda v: _round_amvr(v, j["imv"]) >> rs                          # noqa: E731
    sc = []
    for s in smvd_evaluated_starts(j):
        v = j["starts"][s]
        if s >= j["numFixed"] and j["imv"]:
            v = (_round_amvr(v[0], j["imv"]), _round_amvr(v[1], j["imv"]))
        for i, k in pairs:
            p, q = j["cands"][0][i], j["cands"][1][k]
            bits = _eg_bits(down(v[0]) - down(p[0])) + _eg_bits(down(v[1]) - down(p[1])) + j["idxBits"][i] + j["idxBits"][k]
            sc.append(cost(v, (q[0] - v[0] + p[0], q[1] - v[1] + p[1])) + int(j["lam"] * bits))
    return pc.count(min(pc)), sc.count(min(sc)) if sc else 0
