"""GPU parity of the symmetric-MVD tile kernel (smvd.hip, smvd_tile_kernel) where its wave vote on zero fractions decides: a wave whose active lanes all evaluate
integer vectors on both lists copies the two tiles instead of filtering them (tile_eval_vote), any other wave runs both filter passes.  (32x32 is compiled without
the vote -- registers -- and runs the filters throughout: its cases pin that the two builds of the kernel agree with the oracle on the same vectors.)

  I1  one evaluation per PU (op 0, the vectors set directly) in batches of ONE vector class, so that every wave of the batch lands in one variant: both lists
      integer, x integer only, y integer only, list A integer with list B fractional and the reverse, half-sample positions under the alternative taps (imv 3:
      frac 8 is a filter), zero vectors; every form's smallest shape at 8 and 10 bits; batches of 1, pusPerWave -+ 1 and a few dozen jobs;
  I2  mixed waves: integer PUs with exactly one fractional PU first, in the middle and last of a wave; integer first predictors with fractional second ones (the
      slots of one pass differ: this is what a one-PU-per-workgroup form can mix);
  I3  the whole search on a scene with an integer pan from integer predictors and start vectors (INIT and STARTS copy, DIAMOND and CROSS filter), the same on the
      hard scene (the search leaves its start), imv 1 and 2 (every candidate integer), and the four-slot group form the levels of a 4K picture launch;
  I4  clipMv: integer vectors beyond the limits at the picture corners, and fractional vectors that clamp to an integer bound on one axis and on both;
  I5  the arithmetic around the prediction: SAD, the clipped target, BCW weights -2 (the wide Hadamard), 3, 5 and 10.

Expected values come from the oracle alone (me_util.smvd_member_results "vo_", me_util.smvd_search_oracle), job by job and bit-exact; the member results hold the
one evaluation (cost of mvCur = starts[0] against mvTar = the first list-1 predictor, the first list-0 predictor being starts[0]).  The launch form is asserted from
vtmhip_smvd_launch_form before the device runs (test_gpu_smvd_forms.check_batch)."""
import functools

import numpy as np
import pytest

import me_util
from test_gpu_smvd_forms import Device, check_batch, group_threshold, hard_scene, job_table, noise_scene, num_cus, oracle_results, tile_form

pytestmark = pytest.mark.gpu

# the smallest shape of each form: 8x8 (group, one tile), 16x8 / 8x16 (group, Hadamard pairs), 16x16 (group, four tiles), 32x32 (one wave per PU; compiled without
# the vote), 64x64 (four waves; 64 tiles: a wave holds one slot's lanes, so its lanes always agree) -- and the workgroup shapes whose waves hold SEVERAL slots of a pass
# and take the vote: 64x16 (one wave per PU, 16 tiles in Hadamard pairs: four slots per wave) and 64x32 (four waves, 32 tiles: two slots per wave).  There a wave
# mixes the candidates of a pass, the lanes of a skipped pair `continue` and the last wave-step of a pass is partly active.
SHAPES = [(8, 8), (16, 8), (8, 16), (16, 16), (32, 32), (64, 64), (64, 16), (64, 32)]
CLASSES = ["integer", "x_integer", "y_integer", "a_integer", "b_integer", "alt_half", "zero"]


@functools.lru_cache(maxsize=None)
def pan_scene(bd=10):
    """the plain synthetic clip: the picture moves by (3, 2) samples per frame, so list 0 (two frames back) matches at (+96, +64) sixteenths and list 1 at (-96, -64)"""
    return me_util.SmvdScene(416, 240, hard=False, bit_depth=bd)


def vec(rng, cls_x, cls_y, unit=16, spread=(10, 6)):
    """a vector near the centre of the search area: per axis "i" = a multiple of `unit` (>= 16: integer), "f" = a fraction of 4, 8 or 12, "h" = the half sample"""
    out = []
    for c, r in zip((cls_x, cls_y), spread):
        if c == "i":
            out.append(int(rng.integers(-r * 16 // unit, r * 16 // unit + 1)) * unit)
        else:
            out.append(int(rng.integers(-r, r + 1)) * 16 + (8 if c == "h" else int(rng.choice([4, 8, 12]))))
    return tuple(out)


def class_vectors(rng, cls, imv):
    """(vector of list A, vector of list B) of a class"""
    unit = max(16, 1 << me_util.AMVR_SHIFT[imv])
    if cls == "zero":
        return (0, 0), (0, 0)
    if cls == "alt_half":      # at least one half-sample component in either vector
        a, b = [("h", "i"), ("i", "h"), ("h", "h")][int(rng.integers(0, 3))], [("h", "i"), ("i", "h"), ("h", "h")][int(rng.integers(0, 3))]
        return vec(rng, *a), vec(rng, *b)
    ax = {"integer": "ii", "x_integer": "if", "y_integer": "fi", "a_integer": "ii", "b_integer": "ff"}[cls]
    bx = {"integer": "ii", "x_integer": "if", "y_integer": "fi", "a_integer": "ff", "b_integer": "ii"}[cls]
    return vec(rng, ax[0], ax[1], unit), vec(rng, bx[0], bx[1], unit)


def class_jobs(scene, size, n, seed, cls, **over):
    """n jobs whose every predictor and start vector is of class `cls`; the one evaluation of op 0 is (starts[0] = the first list-0 predictor, the first list-1
    predictor).  over: fields set in every job."""
    rng = np.random.default_rng(seed)
    w, h = size
    jobs = []
    for _ in range(n):
        imv = 3 if cls == "alt_half" else int(rng.choice([0, 0, 1, 2, 3])) if cls in ("integer", "zero") else 0
        imv = over.get("imv", imv)
        pairs = [class_vectors(rng, cls, imv) for _ in range(4)]
        cands = [[pairs[0][0], pairs[1][0]], [pairs[0][1], pairs[1][1]]]
        starts = [pairs[0][0], pairs[2][0], pairs[3][0]]
        j = dict(w=w, h=h, x=int(rng.integers(0, (scene.W - w) // 4 + 1)) * 4, y=int(rng.integers(0, (scene.H - h) // 4 + 1)) * 4, imv=imv,
                 satd=int(rng.integers(0, 5) != 0), clip=int(rng.integers(0, 3) == 0), bcw=int(rng.choice([4, 4, 4, 4, -2, 3, 5, 10])), num=[2, 2], cands=cands,
                 idxBits=[int(rng.integers(1, 3)), int(rng.integers(1, 4))], lam=float(rng.uniform(2, 40)), starts=starts, numFixed=int(rng.integers(2, 4)),
                 modeBits=int(rng.integers(3, 9)))
        j.update(over)
        jobs.append(j)
    return jobs


def fractions(j):
    """the fractions of op 0's two vectors after clipMv: ((ax & 15, ay & 15), (bx & 15, by & 15))"""
    lim = me_util.smvd_clip_limits(pan_scene(), j)      # the limits depend on the picture size and the PU alone
    return tuple(tuple(min(lim[c][1], max(lim[c][0], v[c])) & 15 for c in range(2)) for v in (j["starts"][0], j["cands"][1][0]))


def run_batches(ctx, name, scene, size, jobs, counts=None):
    """the jobs as uniform batches of the given sizes (default: all of them), all four ops against the oracle"""
    exp = oracle_results(scene, jobs)
    table = job_table(scene, jobs)
    dev = Device(ctx, scene)
    for n in sorted(counts or {len(jobs)}):
        check_batch(ctx, dev, name, table, jobs, exp, n, size, True, tile_form(size))
    dev.free()


# ---- I1: one class per batch --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_one_vector_class_per_batch(ctx, size, bd):
    """I1: seven batches per shape and bit depth, each of one class: the copy form for "integer" and "zero" (imv 3 among them: frac 0 is the identity under the
    alternative taps too), the filters for every other class -- a vote taken on list A alone, on one axis alone, or a copy taken for a half-sample vector under
    imv 3 each give another cost here.  Batches of 1, pusPerWave - 1, pusPerWave + 1 and all jobs."""
    scene = pan_scene(bd) if size[0] > 16 else hard_scene(bd)
    ppw = tile_form(size)[3]
    m = 2 * ppw + 3 if ppw > 1 else 6
    for ci, cls in enumerate(CLASSES):
        jobs = class_jobs(scene, size, m, 41000 + size[0] * 131 + size[1] + bd * 7 + ci, cls)
        want = {"integer": lambda f: f == ((0, 0), (0, 0)), "zero": lambda f: f == ((0, 0), (0, 0)), "x_integer": lambda f: f[0][0] == f[1][0] == 0 and f[0][1] and f[1][1],
                "y_integer": lambda f: f[0][1] == f[1][1] == 0 and f[0][0] and f[1][0], "a_integer": lambda f: f[0] == (0, 0) and f[1][0] and f[1][1],
                "b_integer": lambda f: f[1] == (0, 0) and f[0][0] and f[0][1], "alt_half": lambda f: set(f[0] + f[1]) == {0, 8} or set(f[0] + f[1]) == {8}}[cls]
        assert all(want(fractions(j)) for j in jobs), (cls, [fractions(j) for j in jobs])
        run_batches(ctx, "I1 %dx%d %d bits %s" % (size + (bd, cls)), scene, size, jobs, {1, max(1, ppw - 1), ppw + 1, m})


# ---- I2: mixed waves ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_one_fractional_pu_in_a_wave(ctx, size):
    """I2: three waves of integer PUs, the PU at the first, a middle and the last position of its wave replaced in turn by one whose list-B vector is fractional
    (list A stays integer, and so does every lane before it): the wave must filter -- for ALL its PUs the result is the same either way, for the odd one only if
    the vote saw it.  One PU per workgroup above 16x16: there the odd PU is a workgroup of its own."""
    scene = hard_scene()
    ppw = tile_form(size)[3]
    n = 3 * ppw
    base = class_jobs(scene, size, n, 42000 + size[0] * 131 + size[1], "integer", imv=0)
    odd = class_jobs(scene, size, n, 42500 + size[0] * 131 + size[1], "a_integer")
    for pos in sorted({0, ppw + ppw // 2, n - 1}):
        jobs = list(base)
        jobs[pos] = odd[pos]
        assert [fractions(j) != ((0, 0), (0, 0)) for j in jobs] == [k == pos for k in range(n)]
        run_batches(ctx, "I2 %dx%d odd PU at %d" % (size + (pos,)), scene, size, jobs)


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_fractional_second_predictors(ctx, size):
    """I2: the first predictor of either list (and every start vector) integer, the second ones fractional: slot 0 of the INIT pass, and the first tiles' lanes of
    every pass, evaluate integer vectors while later slots do not.  In the group forms and in the 64x16 / 64x32 workgroup forms one wave holds both kinds (its first
    lane an integer one: a vote read from the first lane alone copies fractional tiles); at 64x64 a wave holds one slot, at 32x32 no vote is taken."""
    scene = pan_scene()
    n = 2 * tile_form(size)[3] + 1
    jobs = class_jobs(scene, size, n, 43000 + size[0] * 131 + size[1], "integer", imv=0)
    frac = class_jobs(scene, size, n, 43500 + size[0] * 131 + size[1], "b_integer")
    for j, f in zip(jobs, frac):
        j["cands"] = [[j["cands"][0][0], f["cands"][0][1]], [j["cands"][1][0], f["cands"][0][0]]]
        assert all(v & 15 == 0 for v in j["cands"][0][0] + j["cands"][1][0]) and all(v & 15 for v in j["cands"][0][1] + j["cands"][1][1])
    run_batches(ctx, "I2 %dx%d fractional second predictors" % size, scene, size, jobs)


# ---- I3: the whole search -----------------------------------------------------------------------------------------------------------------------------------------------
def pan_jobs(scene, size, n, seed, imv=0, starts=None):
    """integer predictors (the pan's vector and the zero vector in either list) and integer start vectors around the pan"""
    jobs = class_jobs(scene, size, n, seed, "integer", imv=imv, bcw=4, satd=1, clip=0)
    for j in jobs:
        j["cands"] = [[(96, 64), (0, 0)], [(-96, -64), (0, 0)]]
        j["starts"] = starts or [(96, 64), (0, 0), (96 + 64, 64), (96, 64 - 64), (64, 64)]
    return jobs


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_search_from_integer_vectors_integer_pan(ctx, size):
    """I3: the search stays at its integer centre (asserted from the oracle for at least half of the PUs: an 8x8 block's quarter-sample neighbours win now and then
    over the clip's noise, and some PUs overlap its moving square): INIT and STARTS take the copy, DIAMOND and CROSS -- quarter-sample steps -- the filters."""
    scene = pan_scene()
    jobs = pan_jobs(scene, size, 2 * tile_form(size)[3] + 5, 44000 + size[0] * 131 + size[1])
    exp = oracle_results(scene, jobs)
    stay = sum(1 for e in exp[1] if e[0] == (96, 64) and e[1] == (-96, -64))
    print("smvd identity I3 %dx%d: %d of %d searches end on the pan's integer vector" % (size + (stay, len(jobs))))
    assert stay * 2 >= len(jobs), (stay, len(jobs))
    run_batches(ctx, "I3 %dx%d integer pan" % size, scene, size, jobs)


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_search_from_integer_vectors_hard_scene(ctx, size):
    """I3: integer predictors and start vectors on the hard scene: the search leaves its integer start (asserted for at least a third of the PUs), so a PU's passes
    alternate between the two forms"""
    scene = hard_scene()
    jobs = class_jobs(scene, size, 2 * tile_form(size)[3] + 5, 45000 + size[0] * 131 + size[1], "integer", imv=0)
    exp = oracle_results(scene, jobs)
    moved = sum(1 for e in exp[1] if (e[0][0] | e[0][1]) & 15)
    print("smvd identity I3 %dx%d hard: %d of %d searches end on a fractional vector" % (size + (moved, len(jobs))))
    assert moved * 3 >= len(jobs), (moved, len(jobs))
    run_batches(ctx, "I3 %dx%d hard" % size, scene, size, jobs)


@pytest.mark.parametrize("imv", [1, 2])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_search_integer_amvr(ctx, size, imv):
    """I3: cu.imv 1 and 2: stepShift = 2 + imv_shift makes every candidate of every pass an integer vector -- the whole search runs on copies"""
    scene = hard_scene()
    jobs = class_jobs(scene, size, 2 * tile_form(size)[3] + 5, 46000 + size[0] * 131 + size[1] + imv, "integer", imv=imv)
    exp = oracle_results(scene, jobs)
    assert all((v & 15) == 0 for e in exp[1] for v in e[0] + e[1])
    moved = sum(1 for j, e in zip(jobs, exp[1]) if e[0] not in [tuple(c) for c in j["cands"][0]])
    print("smvd identity I3 %dx%d imv %d: %d of %d searches end off their predictors" % (size + (imv, moved, len(jobs))))
    run_batches(ctx, "I3 %dx%d imv %d" % (size + (imv,)), scene, size, jobs)


@pytest.mark.parametrize("size", [(8, 8), (16, 16)], ids=lambda s: "%dx%d" % s)
def test_four_slot_form_integer_and_mixed(ctx, size):
    """I3: the four-slot group form (batches above eight eight-slot waves per compute unit: what a level of a 4K picture launches): a few dozen jobs -- integer ones
    from the pan, and a fractional one every 23rd row, so that most waves copy and some filter -- repeated to threshold + pusPerWave + 1 rows (whole block only)."""
    scene = pan_scene()
    form = tile_form(size, 4)
    base = pan_jobs(scene, size, 37, 47000 + size[0])
    odd = class_jobs(scene, size, 37, 47500 + size[0], "a_integer")
    jobs = [odd[k] if k % 23 == 11 else base[k] for k in range(37)]
    exp = oracle_results(scene, jobs, members=False)
    n = group_threshold(size, num_cus()) + form[3] + 1
    rows = np.arange(n) % len(jobs)
    table = job_table(scene, jobs)
    dev = Device(ctx, scene)
    check_batch(ctx, dev, "I3 %dx%d four slots" % size, table[rows], [jobs[k] for k in rows], (None, [exp[1][k] for k in rows]), n, size, True, form)
    dev.free()


# ---- I4: clipMv ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_clipped_vectors(ctx, size):
    """I4: PUs at the four picture corners over reference margins of noise, their list-A vectors pointing out of the picture: integer vectors beyond the limits
    (clamped, still integer: the copy reads at the CLAMPED position), fractional vectors beyond the limit on x only / y only (the clamped axis becomes integer, the
    other stays fractional: the filters) and on both axes (both fractions become 0: the copy, although the vectors as given are fractional)."""
    scene = noise_scene()
    w, h = size
    rng = np.random.default_rng(48000 + w * 131 + h)
    jobs, kinds = [], []
    for k in range(32):
        right, bottom, kind = k & 1, (k >> 1) & 1, ("int_beyond", "frac_x_beyond", "frac_y_beyond", "frac_both_beyond")[(k >> 2) & 3]
        j = class_jobs(scene, size, 1, 48100 + k, "integer", imv=0)[0]
        j["x"], j["y"] = (scene.W - w) * right, (scene.H - h) * bottom
        lim = me_util.smvd_clip_limits(scene, j)
        out = [lim[0][right] + (1 if right else -1) * int(rng.integers(1, 12)) * 16, lim[1][bottom] + (1 if bottom else -1) * int(rng.integers(1, 12)) * 16]
        inside = [(-1 if right else 1) * int(rng.integers(1, 8)) * 16, (-1 if bottom else 1) * int(rng.integers(1, 6)) * 16]
        fr = [int(rng.choice([4, 8, 12])), int(rng.choice([4, 8, 12]))]
        a = {"int_beyond": (out[0], out[1]), "frac_x_beyond": (out[0] + fr[0], inside[1] + fr[1]), "frac_y_beyond": (inside[0] + fr[0], out[1] + fr[1]),
             "frac_both_beyond": (out[0] + fr[0], out[1] + fr[1])}[kind]
        b = (inside[0], inside[1])
        j["cands"], j["starts"] = [[a, a], [b, b]], [a, a, a]
        f = fractions(j)
        assert f[1] == (0, 0) and (f[0] == (0, 0)) == (kind in ("int_beyond", "frac_both_beyond")), (kind, j, f)
        if kind == "frac_x_beyond":
            assert f[0][0] == 0 and f[0][1] != 0
        if kind == "frac_y_beyond":
            assert f[0][0] != 0 and f[0][1] == 0
        jobs.append(j)
        kinds.append(kind)
    # one kind per batch (a wave in one variant), then all mixed
    for kind in ("int_beyond", "frac_x_beyond", "frac_y_beyond", "frac_both_beyond"):
        run_batches(ctx, "I4 %dx%d %s" % (size + (kind,)), scene, size, [j for j, kd in zip(jobs, kinds) if kd == kind])
    run_batches(ctx, "I4 %dx%d mixed" % size, scene, size, jobs)


# ---- I5: the arithmetic around the prediction ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [dict(satd=0), dict(clip=1), dict(bcw=-2, satd=1, clip=0), dict(bcw=3), dict(bcw=5), dict(bcw=10)],
                         ids=["sad", "clipBiPred", "bcw-2-wide", "bcw3", "bcw5", "bcw10"])
def test_arithmetic_variants_on_copies(ctx, variant):
    """I5: integer vectors in every job (the copy form) with the setting fixed for the whole batch: SAD, the clipped target, the wide Hadamard of BCW weight -2
    (unclipped), BCW weights 3, 5 and 10 -- 8x8, a Hadamard pair shape, 16x16 and 64x16 (a workgroup form that takes the vote: 32x32 does not)"""
    scene = hard_scene()
    for size in ((8, 8), (16, 8), (16, 16), (64, 16)):
        jobs = class_jobs(scene, size, 2 * tile_form(size)[3] + 3, 49000 + size[0] * 131 + size[1], "integer", **variant)
        run_batches(ctx, "I5 %dx%d %s" % (size + (variant,)), scene, size, jobs)
