"""GPU parity of joint Cb-Cr residual coding (JCCR / ICT): the two pointer entries, the batched forward ICT with the candidate selection, and the fused
joint chain on its three launch paths at 8 / 10 / 12 bits -- against the numpy restatement of the reference's rules (tests/jccr_util.py, itself pinned to
the real templates in tests/test_jccr.py), the recorded reference results (tests/golden/jccr.npz) and the oracle's transform steps.  Bit-exact."""
import ctypes as C
import itertools

import numpy as np
import pytest

import jccr_util as ju
import oracle_lib as ol
from vtm_amd import lib
from vtm_amd.device import ict_select
from vtm_amd.lib import IctJob, JccrJob, JccrResult, TuJob, TuResult, VtmHipError

pytestmark = pytest.mark.gpu

POINTER_SHAPES = [(2, 2), (2, 8), (4, 4), (8, 4), (4, 16), (16, 16)]   # (w, h)


def _strided(rng, blk, extra):
    """blk inside a wider buffer of random samples: a 2-D view whose row stride is wider than the block"""
    h, w = blk.shape
    buf = rng.integers(-32768, 32768, (h, w + extra)).astype(np.int16)
    buf[:, 1:1 + w] = blk
    return buf, buf[:, 1:1 + w]


def _check_pointer_entries(ctx, rng, mode, cb, cr):
    exp_j, exp_d = ju.fwd_ict(mode, cb, cr)
    bcb, vcb = _strided(rng, cb, 3)
    bcr, vcr = _strided(rng, cr, 5)
    got_j, got_d = ctx.fwdTransformCbCr(mode, vcb, vcr)
    assert got_d == exp_d, ("dist", mode, cb.shape, got_d, exp_d)
    assert mode == 0 or np.array_equal(got_j, exp_j), ("joint", mode, cb.shape)
    keep_cb, keep_cr = bcb.copy(), bcr.copy()
    ecb, ecr = ju.inv_ict(mode, cb, cr)
    ctx.invTransformCbCr(mode, vcb, vcr)
    assert np.array_equal(vcb, ecb) and np.array_equal(vcr, ecr), ("inv", mode, cb.shape)
    bcb[:, 1:1 + cb.shape[1]], bcr[:, 1:1 + cb.shape[1]] = cb, cr
    assert np.array_equal(bcb, keep_cb) and np.array_equal(bcr, keep_cr), "samples outside the block were touched"


def test_pointer_entries_match_the_rules(ctx):
    """vtmhip_fwdTransformCbCr / vtmhip_invTransformCbCr, the seven slots of m_fwdICT / m_invICT: strides wider than the block, the whole int16 range (so
    Pel wraps: (4 * 32767 + 2 * 32767) / 5 = 39320), negative odd sums (truncation, not floor) and -32768 under mode -2."""
    rng = np.random.default_rng(41)
    for mode in ju.MODES:
        for (w, h) in POINTER_SHAPES:
            for amp in (5, 1023, 32767):
                cb, cr = ju.random_pair(rng, w, h, amp, full_range=amp == 32767)
                if amp == 32767:
                    cb[0, 0], cr[0, 0] = 32767, (32767 if mode >= 0 else -32767)        # the joint residual wraps
                    cb[0, 1], cr[0, 1] = -3, (-1 if mode >= 0 else 1)                    # 4 * -3 + 2 * -1 = -14: -14 / 5 = -2, floor would give -3
                    cb[1, 0], cr[1, 0] = -32768, 12345                                   # mode -2: the clip of the inverse
                    cb[1, 1], cr[1, 1] = -2, (-1 if mode >= 0 else 1)                    # (-2 + -1) / 2 = -1, floor would give -2
                _check_pointer_entries(ctx, rng, mode, cb, cr)
    with pytest.raises(VtmHipError):
        ctx.fwdTransformCbCr(4, np.zeros((4, 4), np.int16), np.zeros((4, 4), np.int16))
    with pytest.raises(VtmHipError):
        ctx.invTransformCbCr(-4, np.zeros((4, 4), np.int16), np.zeros((4, 4), np.int16))


def test_pointer_entries_replay_the_recorded_reference(ctx):
    for mode, cb, cr, joint, dist, inv in ju.golden_cases():
        got_j, got_d = ctx.fwdTransformCbCr(mode, cb, cr)
        assert got_d == dist and (mode == 0 or np.array_equal(got_j, joint)), (mode, cb.shape)
        a, b = cb.copy(), cr.copy()
        ctx.invTransformCbCr(mode, a, b)
        assert np.array_equal(a if abs(mode) == 3 else b, inv) and np.array_equal(b if abs(mode) == 3 else a, cr if abs(mode) == 3 else cb), ("inv", mode, cb.shape)


def _ict_batch_data():
    """~1000 mixed (Cb, Cr) pairs inside one plane: the small ones (height <= 8) in 8-row bands of their own, the tall ones over a shared region"""
    rng = np.random.default_rng(43)
    shapes = [(2, 2), (2, 8), (4, 4), (8, 4), (4, 8), (8, 8), (16, 4), (4, 16), (16, 16), (32, 8), (32, 32), (64, 64), (1, 4), (8, 1)]
    n, stride = 1008, 72
    resi = rng.integers(-32768, 32768, (n * 8, 2 * stride)).astype(np.int16)   # small pairs: 8 rows each; the big ones get their own plane below
    big = rng.integers(-1023, 1024, (64 * 24, 2 * stride)).astype(np.int16)
    plane = np.concatenate([resi, big])
    jobs = (IctJob * n)()
    pairs, out_off, nbig = [], 0, 0
    for k in range(n):
        w, h = shapes[k % len(shapes)]
        if h > 8:
            if nbig >= 24 * 64 // h:
                w, h = 8, 8
            else:
                row = n * 8 + nbig * h
                nbig += 1
        if h <= 8:
            row = k * 8
            amp = int(rng.choice([4, 90, 1023, 32767]))
            cb, cr = ju.random_pair(rng, w, h, amp, full_range=amp == 32767)
            if k % 5 == 0:
                cr = ju._pel(np.clip((1 - 2 * (k % 2)) * cb.astype(np.int64) * int(rng.integers(1, 5)) // 4, -32768, 32767))   # correlated: a joint mode wins
            plane[row:row + h, 2:2 + w], plane[row:row + h, stride + 3:stride + 3 + w] = cb, cr
        cb, cr = plane[row:row + h, 2:2 + w].copy(), plane[row:row + h, stride + 3:stride + 3 + w].copy()
        j = jobs[k]
        j.cbOff, j.crOff, j.cbStride, j.crStride = row * 2 * stride + 2, row * 2 * stride + stride + 3, 2 * stride, 2 * stride
        j.width, j.height, j.signFlag, j.maskBits, j.outOff = w, h, k % 2, (2 * (k % 8)) & 14, out_off
        pairs.append((cb, cr, out_off))
        out_off += 3 * w * h
    return plane, jobs, pairs, n, out_off


def test_ict_fwd_batch_and_selection(ctx):
    """~1000 mixed pairs in one launch: the four (d1, d2) pairs, every requested joint plane (and no other), and selectICTCandidates on the device's
    distances for inter and intra CUs."""
    plane, jobs, pairs, n, out_off = _ict_batch_data()
    d_plane, d_jobs = ctx.to_device(plane), ctx.to_device(np.frombuffer(jobs, np.uint8))
    d_joint, d_dist = ctx.to_device(np.full(out_off, 0x5555, np.int16)), ctx.alloc(64 * n)
    ctx.ict_fwd_batch(d_plane.ptr, d_jobs.ptr, n, d_dist.ptr, d_joint.ptr)
    dist, joint = d_dist.to_host(np.int64).reshape(n, 4, 2), d_joint.to_host(np.int16)
    two = 0
    for k, (cb, cr, off) in enumerate(pairs):
        wh = cb.size
        for m in range(4):
            ej, ed = ju.fwd_ict(ju.mode_of(jobs[k].signFlag, m), cb, cr)
            assert tuple(int(v) for v in dist[k, m]) == ed, (k, m, cb.shape)
            if m:
                got = joint[off + (m - 1) * wh:off + m * wh]
                if (jobs[k].maskBits >> m) & 1:
                    assert np.array_equal(got, ej.reshape(-1)), ("plane", k, m, cb.shape)
                else:
                    assert (got == 0x5555).all(), ("plane not asked for", k, m)
        for intra in (0, 1):
            sel = ict_select(dist[k], intra)
            assert sel == ju.select_ict(dist[k], intra), (k, intra)
            two += len(sel) == 2
    assert two > 20   # the intra rule's second candidate is exercised by the data
    ctx.ict_fwd_batch(d_plane.ptr, d_jobs.ptr, 0, d_dist.ptr, d_joint.ptr)   # n == 0
    # no plane buffer: distances only
    d_dist2 = ctx.alloc(64 * n)
    ctx.ict_fwd_batch(d_plane.ptr, d_jobs.ptr, n, d_dist2.ptr, None)
    assert np.array_equal(d_dist2.to_host(np.int64).reshape(n, 4, 2), dist)


# ---- the joint chain ----------------------------------------------------------------------------------------------------------------------------
GENERIC_SHAPES = [(2, 2), (2, 8), (4, 4), (8, 4), (4, 8), (8, 8), (16, 4), (4, 16), (16, 16), (32, 8), (32, 32), (64, 64)]
LANE_SHAPES = [(4, 4), (8, 4), (4, 8)]
BLOCKED_SHAPES = [(8, 8), (16, 16), (32, 8), (32, 32)]
SIGNED_MODES = [1, -1, 2, -2, 3, -3]

_batches = {}


def _recipe_batch(kind, bd):
    """The issue's input recipe, every (amplitude, QP, mode) combination (96 of them) equally often, shuffled over the shapes: computed once per (path, depth)."""
    if (kind, bd) in _batches:
        return _batches[(kind, bd)]
    shapes = {"generic": GENERIC_SHAPES, "lane": LANE_SHAPES, "blocked": BLOCKED_SHAPES}[kind]
    rng = np.random.default_rng(1000 * bd + len(kind))
    grid = list(itertools.product([8, 60, 400, (1 << bd) - 1], [22, 27, 32, 37], SIGNED_MODES))
    reps = {"generic": 2, "lane": 3, "blocked": 4}[kind]          # 192 / 288 / 384 jobs: 16 / 96 / 96 per shape
    combos = [grid[i] for r in range(reps) for i in rng.permutation(len(grid))]
    specs = []
    for k, (amp, qp, mode) in enumerate(combos):
        w, h = shapes[k % len(shapes)]
        cb, cr = ju.recipe_pair(rng, w, h, bd, amp, mode)
        q = qp + 6 * (bd - 8)
        ts = kind == "generic" and (k + k // len(shapes)) % 4 == 3 and w <= 32 and h <= 32   # every fourth job of every shape
        specs.append((cb, cr, ju.mask_of(mode), int(mode < 0), q // 6, q % 6, int(rng.integers(0, 2)), ts))
    _batches[(kind, bd)] = ju.ChainBatch(specs, bd, cb_col=5 if (kind, bd) == ("lane", 8) else 4)   # one lane batch on rows that are not 8-byte aligned
    return _batches[(kind, bd)]


def _assert_recipe_discriminates(batch):
    share = batch.coded_share()
    assert share >= 0.40 and 1.0 - share >= 0.10, share   # on the EXPECTED values: enough coded jobs and enough all-zero ones


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_jccr_chain_generic_path(ctx, bd):
    """One mixed launch over sides 2 .. 64 on the LDS kernel, every fourth job (sides <= 32) a transform-skip job."""
    b = _recipe_batch("generic", bd)
    _assert_recipe_discriminates(b)
    assert sum(j.typeHor == ju.TRSKIP for j in b.jobs) >= 30
    b.check(b.run(ctx, 64, 64))
    # the 64-threads-per-pair variant of the same kernel (maxWidth * maxHeight <= 256) on the jobs that fit
    small = [k for k, (w, h) in enumerate(b.shapes) if w <= 16 and h <= 16]
    b.check(b.run(ctx, 16, 16, idx=small), idx=small)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_jccr_chain_lane_path(ctx, bd):
    """uniformSize launches of 4x4, 8x4, 4x8: one lane per pair."""
    b = _recipe_batch("lane", bd)
    _assert_recipe_discriminates(b)
    for (w, h) in LANE_SHAPES:
        idx = [k for k, s in enumerate(b.shapes) if s == (w, h)]
        assert len(idx) > 64
        b.check(b.run(ctx, w, h, uniform=True, idx=idx), idx=idx)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_jccr_chain_blocked_path(ctx, bd):
    """uniformSize launches of 8x8, 16x16, 32x8, 32x32: the register-blocked kernel (4 .. 64 lanes per pair, several workgroups, a ragged last one)."""
    b = _recipe_batch("blocked", bd)
    _assert_recipe_discriminates(b)
    for (w, h) in BLOCKED_SHAPES:
        idx = [k for k, s in enumerate(b.shapes) if s == (w, h)][:-1]   # 95 jobs: the last workgroup is not full
        b.check(b.run(ctx, w, h, uniform=True, idx=idx), idx=idx)


@pytest.mark.parametrize("bd", [10, 12])
def test_jccr_chain_headroom(ctx, bd):
    """Modes +-1 / +-3 with cb = s * cr = +-(2^bd - 1) and signs along a transform basis row: the joint residual reaches 6 * (2^bd - 1) / 5, beyond the
    +-(2^bd - 1) the plain chain documents, and drives the first pass to its largest values.  Blocked and generic path, sides 8, 32 and 64."""
    rng = np.random.default_rng(90 + bd)
    amp, specs = (1 << bd) - 1, []
    for (w, h) in [(8, 8), (32, 32), (64, 64), (32, 8), (8, 64)]:
        for mode in (1, -1, 3, -3):
            for (rh, rv) in [(0, 0), (1, min(h, 32) - 1), (int(rng.integers(0, min(w, 32))), int(rng.integers(0, min(h, 32))))]:
                cb = ol.basis_sign_block(w, h, 0, 0, rh, rv, amp)
                cr = ((-1 if mode < 0 else 1) * cb.astype(np.int32)).astype(np.int16)
                q = int(rng.choice([22, 37])) + 6 * (bd - 8)
                specs.append((cb, cr, ju.mask_of(mode), int(mode < 0), q // 6, q % 6, 0, False))
    b = ju.ChainBatch(specs, bd)
    assert max(int(np.abs(e["joint"].astype(np.int32)).max()) for e in b.exp) == 6 * amp // 5
    b.check(b.run(ctx, 64, 64))
    for shape in sorted(set(b.shapes)):
        idx = [k for k, s in enumerate(b.shapes) if s == shape]
        b.check(b.run(ctx, shape[0], shape[1], uniform=True, idx=idx), idx=idx)


@pytest.mark.parametrize("shape", [(4, 4), (16, 16), (8, 4)])
def test_jccr_chain_levels_equal_the_plain_chain_on_the_joint_plane(ctx, shape, bd=10):
    """No oracle: the levels (and sumAbs / absSum) of the joint chain equal those of vtmhip_tu_chain_batch_dev run on the joint plane that
    vtmhip_ict_fwd_batch_dev wrote, and its fwdDist equals that call's d1."""
    w, h = shape
    rng = np.random.default_rng(7 + w * h)
    n, stride = 150, 2 * w + 8
    resi = np.zeros((n * h, stride), np.int16)
    ict, jc, tu = (IctJob * n)(), (JccrJob * n)(), (TuJob * n)()
    for k in range(n):
        mode = SIGNED_MODES[k % 6]
        cb, cr = ju.recipe_pair(rng, w, h, bd, int(rng.choice([60, 400, 1023])), mode)
        resi[k * h:(k + 1) * h, 0:w], resi[k * h:(k + 1) * h, w + 4:2 * w + 4] = cb, cr
        mask, sign, q = ju.mask_of(mode), int(mode < 0), int(rng.choice([22, 27, 32])) + 12
        a, b, t = ict[k], jc[k], tu[k]
        a.cbOff, a.crOff, a.cbStride, a.crStride, a.width, a.height, a.signFlag, a.maskBits = k * h * stride, k * h * stride + w + 4, stride, stride, w, h, sign, 1 << mask
        a.outOff = (k * 3 - (mask - 1)) * w * h + 2 * w * h          # the one requested plane of job k lands in slot 3 * k ... whatever the mask
        b.cbOff, b.crOff, b.resiStride, b.outOff, b.width, b.height = a.cbOff, a.crOff, stride, k * w * h, w, h
        b.qpPer, b.qpRem, b.typeHor, b.bitDepth, b.isIRAP, b.cbfMask, b.signFlag = q // 6, q % 6, 0, bd, k % 2, mask, sign
        t.resiOff, t.outOff, t.resiStride, t.width, t.height = (k * 3 + 2) * w * h, k * w * h, w, w, h
        t.qpPer, t.qpRem, t.typeHor, t.typeVer, t.bitDepth, t.isIRAP = q // 6, q % 6, 0, 0, bd, k % 2
    d_resi = ctx.to_device(resi)
    d_joint, d_dist = ctx.to_device(np.zeros((3 * n + 4) * w * h, np.int16)), ctx.alloc(64 * n)
    ctx.ict_fwd_batch(d_resi.ptr, ctx.to_device(np.frombuffer(ict, np.uint8)).ptr, n, d_dist.ptr, d_joint.ptr)
    d_lv_t, d_res_t = ctx.to_device(np.zeros(n * w * h, np.int32)), ctx.alloc(C.sizeof(TuResult) * n)
    ctx.tu_chain_batch(d_joint.ptr, ctx.to_device(np.frombuffer(tu, np.uint8)).ptr, n, w, h, d_res_t.ptr, d_lv_t.ptr, None, uniform=True)
    d_lv_j, d_res_j = ctx.to_device(np.ones(n * w * h, np.int32)), ctx.alloc(C.sizeof(JccrResult) * n)
    ctx.jccr_chain_batch(d_resi.ptr, ctx.to_device(np.frombuffer(jc, np.uint8)).ptr, n, w, h, d_res_j.ptr, d_lv_j.ptr, None, None, uniform=True)
    lv_t, lv_j = d_lv_t.to_host(), d_lv_j.to_host()
    assert np.array_equal(lv_t, lv_j) and np.abs(lv_j).sum() > 0
    rt = (TuResult * n).from_buffer_copy(d_res_t.to_host(np.uint8).tobytes())
    rj = (JccrResult * n).from_buffer_copy(d_res_j.to_host(np.uint8).tobytes())
    dist = d_dist.to_host(np.int64).reshape(n, 4, 2)
    for k in range(n):
        assert (rj[k].sumAbs, rj[k].absSum) == (rt[k].sumAbs, rt[k].absSum) and rj[k].fwdDist == dist[k, jc[k].cbfMask, 0], k


def test_jccr_chain_argument_errors_launch_nothing(ctx):
    """cbfMask outside 1 .. 3 and transform skip on a side > 32 return VTMHIP_E_INVALID; the results keep their sentinel and no chain kernel is launched."""
    resi = np.zeros((64, 160), np.int16)

    def call(mask, w, h, type_hor, n=2, uniform=False, max_wh=(64, 64)):
        jobs = (JccrJob * 2)()
        for k in range(2):
            j = jobs[k]
            j.cbOff, j.crOff, j.resiStride, j.outOff, j.width, j.height = 0, 80, 160, k * 4096, 8, 8
            j.qpPer, j.qpRem, j.typeHor, j.bitDepth, j.isIRAP, j.cbfMask, j.signFlag = 5, 2, 0, 10, 0, 3, 0
        jobs[1].cbfMask, jobs[1].width, jobs[1].height, jobs[1].typeHor = mask, w, h, type_hor
        d_resi, d_jobs = ctx.to_device(resi), ctx.to_device(np.frombuffer(jobs, np.uint8))
        d_res = ctx.to_device(np.full(2 * C.sizeof(JccrResult), 0xA5, np.uint8))
        ctx.kernel_timing(True)
        try:
            st = ctx.L.vtmhip_jccr_chain_batch_dev(ctx.h, d_resi.ptr, d_jobs.ptr, n, max_wh[0], max_wh[1], int(uniform), None, None, None, d_res.ptr)
            launches = sum(ctx.kernel_timing_read(k)[1] for k in ("jccr_chain_kernel", "jccr_chain_lane_kernel", "jccr_chain_uni_kernel"))
        finally:
            ctx.kernel_timing(False)
        return st, launches, bool((d_res.to_host(np.uint8) == 0xA5).all())

    assert call(3, 8, 8, 0) == (lib.OK, 1, False)                       # the table itself is fine
    assert call(0, 8, 8, 0) == (lib.E_INVALID, 0, True)
    assert call(4, 8, 8, 0) == (lib.E_INVALID, 0, True)
    assert call(2, 64, 8, ju.TRSKIP) == (lib.E_INVALID, 0, True)         # transform skip on a side > 32
    assert call(2, 8, 64, ju.TRSKIP) == (lib.E_INVALID, 0, True)
    assert call(2, 32, 32, ju.TRSKIP) == (lib.OK, 1, False)
    assert call(2, 8, 8, 1) == (lib.E_INVALID, 0, True)                  # DCT-8: not a joint chroma candidate
    assert call(2, 16, 16, 0, uniform=True, max_wh=(8, 8)) == (lib.E_INVALID, 0, True)   # a uniform launch with a job of another shape
    assert call(0, 8, 8, 0, n=0) == (lib.OK, 0, True)                    # n == 0: nothing read, nothing launched
    assert ctx.L.vtmhip_jccr_chain_batch_dev(ctx.h, None, None, 2, 64, 64, 0, None, None, None, None) == lib.E_INVALID
