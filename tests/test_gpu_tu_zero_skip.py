"""The fused chain leaves the inverse transform out where no level is non-zero (the reference's `if( currAbsSum > 0 )` around invTransformNxN): the decision
is taken per wave (lane groups of up to 64 lanes) or per workgroup (128 / 256 lanes), so every test here mixes TUs with and without levels at the places
where the two granularities differ.  Expectations: the oracle's separate steps (tu_skip_util.Tu); compared: sse, sumAbs, absSum, every level, every
reconstructed sample (the buffers are pre-filled with a sentinel: a skipped TU must still write its zeros), then once more without levels / rec buffers.

"Zero" TUs: amplitude +-3 at QP 37; "non-zero" TUs: amplitude 400 -- at 10 bits.  At 8 and 12 bits the QP moves by 6 per bit as the driver's does, so the
quantiser step keeps its size relative to full scale, and the two amplitudes move with full scale too (1 and 100 at 8 bits, 12 and 1600 at 12 bits);
whether a TU is "zero" is decided by the oracle's absSum, asserted before any launch.  Batches of 2 * (TUs per workgroup) + 3 TUs: the last workgroup is partial."""
import numpy as np
import pytest

import oracle_lib as ol
import tu_skip_util as tu

pytestmark = pytest.mark.gpu

QP = 37


def amps(bd):
    """(zero, non-zero) amplitudes of the depth"""
    return max(1, 3 << bd >> 10), 400 << bd >> 10


# (w, h, uniform, TUs per workgroup, TUs per wave): one per lane-group form of tu_chain_uni_kernel, the one-lane kernel, and the generic kernel (64 threads per
# TU below 257 samples, 256 above) through a call that does not promise one size
FORMS = {
    "8x8_lpt4": (8, 8, True, 64, 16), "16x8_lpt8": (16, 8, True, 32, 8), "16x16_lpt16": (16, 16, True, 16, 4), "32x16_lpt32": (32, 16, True, 8, 2),
    "32x32_lpt64": (32, 32, True, 4, 1), "64x32_lpt128": (64, 32, True, 2, 1), "64x64_lpt256": (64, 64, True, 1, 1), "4x4_lane": (4, 4, True, 256, 64),
    "generic64": (16, 16, False, 4, 1), "generic256": (64, 64, False, 1, 1),
}
GENERIC_SHAPES = {"generic64": [(16, 16), (8, 8), (16, 8), (4, 8), (8, 16), (4, 4), (16, 4)], "generic256": [(64, 64), (32, 32), (64, 32), (16, 64), (32, 16)]}


def _shape(form, k):
    w, h, uniform, _tpw, _tpv = FORMS[form]
    return (w, h) if uniform else GENERIC_SHAPES[form][k % len(GENERIC_SHAPES[form])]


_pools = {}


def pools(form, bd):
    """(zero TUs, non-zero TUs), one of each per batch position, computed once"""
    if (form, bd) not in _pools:
        n = 2 * FORMS[form][3] + 3
        rng = np.random.default_rng(9000 + 16 * sorted(FORMS).index(form) + bd)
        az, an = amps(bd)
        z, nz = [], []
        for k in range(n):
            w, h = _shape(form, k)
            th, tv = tu.types_of(w, h, k)
            z.append(tu.Tu(rng.integers(-az, az + 1, (h, w)), bd, QP, th, tv, irap=k & 1))
            nz.append(tu.Tu(rng.integers(-an, an + 1, (h, w)), bd, QP, th, tv, irap=k & 1))
        assert all(t.absSum == 0 for t in z) and all(t.absSum > 0 for t in nz)
        assert all(t.sse > 0 for t in z)
        _pools[(form, bd)] = (z, nz)
    return _pools[(form, bd)]


def patterns(n, tpw, tpv):
    """name -> the positions of the non-zero TUs"""
    second_wave = tpv if tpw > tpv else 1   # the first TU of a workgroup's second wave (or, one TU per workgroup, of the second workgroup)
    return {
        "all zero": [], "none zero": list(range(n)),
        "first of a wave": [0], "last of a wave": [tpv - 1], "second wave of a workgroup": [second_wave],
        "alternating": list(range(0, n, 2)), "alternating, odd": list(range(1, n, 2)),
        "last job non-zero, dead groups behind it": [n - 1], "last job zero after a non-zero one": [n - 2],
    }


def launch(ctx, form, tus, tag):
    w, h, uniform, _tpw, _tpv = FORMS[form]
    tu.run_check(ctx, tus, w, h, uniform, tag=(form, tag))


@pytest.mark.parametrize("bd", [10, 8, 12])
@pytest.mark.parametrize("form", list(FORMS))
def test_zero_and_coded_tus_side_by_side(ctx, form, bd):
    z, nz = pools(form, bd)
    n = len(z)
    assert n < 256 or FORMS[form][2]      # the call without the size promise stays below the batch size that buckets by shape
    for name, at in patterns(n, FORMS[form][3], FORMS[form][4]).items():
        launch(ctx, form, [nz[k] if k in at else z[k] for k in range(n)], (bd, name))


def _first_level(unit, bd):
    """The amplitude a at which the block a * unit (unit: +-1 per sample) first gets a level (the oracle decides): returns (Tu at a, Tu at a - 1)."""
    prev = None
    for a in range(1, 1 << bd):
        t = tu.Tu(a * unit, bd, QP)
        if t.absSum:
            return t, prev
        prev = t
    raise AssertionError("no amplitude of the depth is coded")


@pytest.mark.parametrize("form", [f for f in FORMS if FORMS[f][2]])
def test_one_level_of_magnitude_one_against_none(ctx, form, bd=10):
    """absSum exactly 1 beside the same block one amplitude step lower (absSum 0), in one wave and in a wave (workgroup) of its own.  The one level is the DC
    (a constant block of either sign: the first lane of the group quantises it) or the first horizontal frequency (the signs of row 1 of the matrix: another
    lane does, so a decision that listens to one lane only misses it)."""
    w, h, _u, tpw, _tpv = FORMS[form]
    z, _nz = pools(form, bd)
    n = len(z)
    ones = np.ones((h, w), np.int64)
    for sign, unit, at in ((1, ones, 0), (-1, -ones, 0), (0, ol.basis_sign_block(w, h, 0, 0, 1, 0, 1).astype(np.int64), 1)):
        one, none = _first_level(unit, bd)
        assert one.absSum == 1 and none is not None and none.absSum == 0 and none.sse > 0 and one.levels[at] in (1, -1)
        tus = list(z)
        tus[1], tus[2], tus[n - 1] = one, none, none
        tus[tpw], tus[tpw + 1] = none, one
        launch(ctx, form, tus, ("absSum 1 / 0", sign))
        launch(ctx, form, [none] * (n - 1) + [one], ("absSum 1 last", sign))
        launch(ctx, form, [none] * n, ("absSum 0", sign))


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_checkerboard_64x64_has_no_level_and_a_large_sse(ctx, bd):
    """+-(2^bd - 1) alternating by sample: all its energy lies in the frequencies the 64-point transform zeroes out, so no level is coded and the SSE is
    sum resi^2 = 4096 (2^bd - 1)^2: 4 286 582 784 at 10 bits (beyond 2^31), 68 685 926 400 at 12 (beyond 2^32)."""
    m = (1 << bd) - 1
    y, x = np.mgrid[0:64, 0:64]
    cb = tu.Tu(np.where((x + y) & 1, -m, m), bd, QP)
    assert cb.absSum == 0 and cb.sse == 4096 * m * m and cb.sse > (0, 0, 1 << 31, 0, 1 << 32)[bd - 8] and not cb.rec.any()
    coded = pools("64x64_lpt256", bd)[1]
    for form in ("64x64_lpt256", "generic256"):
        launch(ctx, form, [cb] * 5, (bd, "checkerboards"))
        launch(ctx, form, [cb, coded[0], cb, cb, coded[1]], (bd, "checkerboards and coded TUs"))


@pytest.mark.parametrize("form", ["8x8_lpt4", "32x32_lpt64", "64x32_lpt128", "4x4_lane", "generic64"])
def test_chroma_residual_scaling_with_a_non_unit_adj(ctx, form, bd=10, adj=1500):
    """The CRS chains (unit scale: 2048): a skipped TU is inv( 0 ) = 0, its SSE is taken against the unscaled residual."""
    w, h, uniform, tpw, tpv = FORMS[form]
    n = 2 * tpw + 3
    rng = np.random.default_rng(31 + w * h)
    z = [tu.Tu(rng.integers(-3, 4, _shape(form, k)[::-1]), bd, QP, adj=adj) for k in range(n)]
    nz = [tu.Tu(rng.integers(-400, 401, _shape(form, k)[::-1]), bd, QP, adj=adj if k % 3 else 0) for k in range(n)]
    assert all(t.absSum == 0 for t in z) and all(t.absSum > 0 for t in nz)
    pats = patterns(n, tpw, tpv)
    for name in ("all zero", "alternating", "last of a wave", "last job non-zero, dead groups behind it"):
        tu.run_check(ctx, [nz[k] if k in pats[name] else z[k] for k in range(n)], w, h, uniform, crs=True, tag=(form, name))
