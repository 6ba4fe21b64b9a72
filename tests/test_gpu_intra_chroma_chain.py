"""GPU parity of vtmhip_intra_chroma_chain_batch_dev: both chroma predictions, their residuals, the single-component and the joint Cb-Cr chain with chroma residual
scaling, the clipped reconstructions and their SSE in one call.  Bit-exact, no tolerance.
Expectation A is composed (intra_chroma_chain_util.Level.expect) from entries that are pinned to the reference -- vtmhip_intra_chroma_pred_batch_dev,
vtmhip_tu_chain_crs_batch_dev / vtmhip_jccr_chain_crs_batch_dev with uniformSize == 0 on the uploaded residual -- with the residual, the reconstruction and the int64
SSE in numpy.  Expectation B covers the jobs on 4x4, 8x8 and 16x16 blocks with cclm_util.predict and lmcs_util.tu_chain_expect / jccr_chain_expect on the CPU
oracle, so one case per lane path rests on nothing the device computes.
Every buffer is compared in full: the lines lie between runs of 0x7fff, the originals at odd offsets with stride 97, and every prediction and output block between
samples of fill that must stay."""
import numpy as np
import pytest

import cclm_util as cu
import intra_chroma_chain_util as ccu
from vtm_amd import lib
from vtm_amd.device import struct_array_to_numpy
from vtm_amd.lib import DistJob, VtmHipError

pytestmark = pytest.mark.gpu

QPS = (10, 27, 38, 51)
M7 = [0, 1, 2, 18, 34, 50, 66]
KINDS = ("random", "alt", "swing", "random", "random")


def shapes_of(sizes, n, rot=0, extra_modes=0):
    """n blocks over `sizes`: bit depth, plane kind, availability class, collocated and first-row rotating; two or three regular modes and one LM mode each (rot
    turns the LM modes against the availability classes); the last block has constant lines and luma and an original within 1 of them"""
    out = []
    for k in range(n):
        w, h = sizes[k % len(sizes)]
        modes = [M7[(k + 3 * j) % 7] for j in range(2 + extra_modes)] + [67 + (k + rot) % 3]
        out.append((w, h, (8, 10, 12)[k % 3], "const" if k == n - 1 else KINDS[k % 5], cu.AVAIL_CLASSES[(k + k // 6) % 6], (k + k // 3) % 2 == 1, k % 4 >= 2, modes))
    return out


def cands(ts=True, adjs=ccu.ADJS, many=0):
    """every second prediction takes all its candidates (Cb / Cr x DCT2 / transform skip, three masks x the transforms), the others 1 .. 4 single and 0 .. 6 joint
    ones; many: that many QPs per single candidate"""
    def f(p, b):
        sc = [(0, 0), (1, 0)] + ([(0, 1), (1, 1)] if ts else [])
        jc = [(m, t) for t in ((0, 1) if ts else (0,)) for m in (1, 2, 3)]
        ns, nj = (len(sc), len(jc)) if p % 2 == 0 else (1 + p % len(sc), p % (len(jc) + 1))
        qp = lambda k: 45 if b["kind"] == "const" else QPS[(p + k) % 4]      # noqa: E731
        single = [(c, t, qp(k), (p + k) & 1, adjs[(p + k) % len(adjs)]) for k, (c, t) in enumerate(sc[:ns])]
        if many:
            single = [(c, t, 20 + 2 * q + (p & 1), irap, adj) for c, t, _, irap, adj in single for q in range(many)]
        return single, [(m, (p + k) & 1, t, qp(k + 1), (p + k) & 1, adjs[(p + 2 * k) % len(adjs)]) for k, (m, t) in enumerate(jc[:nj])]
    return f


NONZERO = ccu.ADJS[1:]
# what each case reaches: lanes per prediction / single chain / joint chain / finish lanes / CRS instantiations
CASES = {
    "4x4": (shapes_of([(4, 4)], 7), cands(ts=False, adjs=(0,))),                                       # 16 / one lane per TU / the same / 16 / plain
    "8x4": (shapes_of([(8, 4)], 6, 1), cands(ts=False, adjs=NONZERO)),                                    # 16 / one lane per TU <8, 4> / the same / 16 / CRS
    "4x8": (shapes_of([(4, 8)], 6, 2), cands(ts=False)),                                                  # 16 / one lane per TU <4, 8> / the same / 16 / CRS
    "8x8": (shapes_of([(8, 8)], 7, 1), cands(ts=False, adjs=NONZERO)),                                    # 16 / register-blocked / jccr_chain_uni_kernel / 16 / CRS
    "16x16": (shapes_of([(16, 16)], 7, 2), cands(ts=False)),                                              # 64 / register-blocked / the same / 16 / CRS
    "large": (shapes_of([(32, 32), (32, 16)], 5), cands()),                                            # 64 / generic at 256 lanes / the same / 64 / CRS
    "small-ts": (shapes_of([(4, 4), (8, 8), (16, 16), (16, 4), (4, 16), (8, 4)], 7, 1), cands()),         # 64 / generic at 64 lanes / the same / 16 / CRS
    "bucketed": (shapes_of([(8, 8), (16, 16), (16, 8), (8, 16)], 4, 2, 1), cands(adjs=NONZERO, many=6)),  # 64 / bucketed by shape / generic at 64 lanes / 16 / CRS
}
PATHS = {"4x4": (16, "lane", "lane", 16, 0), "8x4": (16, "lane", "lane", 16, 1), "4x8": (16, "lane", "lane", 16, 1), "8x8": (16, "blocked", "blocked", 16, 1),
         "16x16": (64, "blocked", "blocked", 16, 1), "large": (64, "generic256", "generic256", 64, 1), "small-ts": (64, "generic64", "generic64", 16, 1),
         "bucketed": (64, "bucketed", "generic64", 16, 1)}


@pytest.fixture(scope="module")
def levels():
    """the tables of every case, built once; Level.expect caches the composed expectation"""
    return {k: ccu.make_level(np.random.default_rng(500 + i), shapes, cand) for i, (k, (shapes, cand)) in enumerate(CASES.items())}


def test_the_cases_reach_every_path(levels):
    assert {k: lv.paths() for k, lv in levels.items()} == PATHS
    assert levels["bucketed"].n_tu >= 256 and levels["small-ts"].n_tu < 256 and levels["small-ts"].n_joint < 256
    assert all(min(b["w"], b["h"]) >= 8 for b in levels["bucketed"].blocks)
    allv = list(levels.values())
    blocks = [b for lv in allv for b in lv.blocks]
    assert {b["bd"] for b in blocks} == {8, 10, 12} and {b["first_row"] for b in blocks} == {False, True} and {b["coloc"] for b in blocks} == {False, True}
    assert {(b["above"], b["left"]) for b in blocks} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(0 < b["ar"] < b["w"] for b in blocks) and any(b["ar"] == b["w"] for b in blocks) and any(b["bl"] == b["h"] for b in blocks)
    assert {lv.job_arr[k].mode for lv in allv for k in range(lv.n_pred)} == set(M7) | {67, 68, 69}
    lm_classes = {(lv.job_arr[k].mode, lv.blocks[lv.job_arr[k].block]["above"], lv.blocks[lv.job_arr[k].block]["left"]) for lv in allv for k in range(lv.n_pred)
                  if lv.job_arr[k].mode >= 67}
    assert len(lm_classes) == 12                                              # each LM mode under each of the four (above, left) combinations
    tu = [t for lv in allv for t in lv.tables()[2]]
    jt = [t for lv in allv for t in lv.tables()[3]]
    assert {(t.component, t.typeHor) for t in tu} == {(c, th) for c in (0, 1) for th in (lib.DCT2, lib.TRSKIP)} and {t.isIRAP for t in tu + jt} == {0, 1}
    assert {(t.cbfMask, t.signFlag, t.typeHor) for t in jt} == {(m, s, th) for m in (1, 2, 3) for s in (0, 1) for th in (lib.DCT2, lib.TRSKIP)}
    assert {t.chromaAdj for t in tu} == set(ccu.ADJS) and {t.chromaAdj for t in jt} == set(ccu.ADJS)
    assert any(t.typeHor == lib.TRSKIP and lv.block_of_pred(t.pred)["w"] == 32 for lv in allv for t in lv.tables()[2] + lv.tables()[3])
    for lv in allv:
        assert max(np.bincount([t.pred for t in lv.tables()[3]])) == (6 if any(j[3] for j in lv.joints) else 3)


@pytest.mark.parametrize("case", list(CASES))
def test_path_matrix(ctx, levels, case):
    lv = levels[case]
    exp = lv.expect(ctx)
    for abs_sums in ([r[3] for r in exp["results"]], [r[6] for r in exp["jres"]]):
        assert min(abs_sums) == 0 and max(abs_sums) > 0                       # on the expected values: a cbf of 0 and of 1 both occur in each table
    got = lv.run(ctx)
    lv.check(got, exp)
    if case in ("4x4", "8x8", "16x16"):                                        # without any device entry: the restatements and the oracle
        ks, kj = list(range(0, lv.n_tu, max(1, lv.n_tu // 24))), list(range(0, lv.n_joint, max(1, lv.n_joint // 24)))
        assert len(ks) >= 8 and len(kj) >= 8
        assert {lv.job_arr[lv.tu_arr[k].pred].mode >= 67 for k in ks} == {False, True} and {lv.job_arr[lv.joint_arr[k].pred].mode >= 67 for k in kj} == {False, True}
        for k in ks:
            lv.check_oracle_single(got, k)
        for k in kj:
            lv.check_oracle_joint(got, k)


def test_sse_is_what_the_distortion_entry_gives(ctx, levels):
    lv = levels["small-ts"]
    got = lv.run(ctx)
    items = [(lv.tu_arr[k].pred, lv.tu_arr[k].component, lv.tu_arr[k].outOff, 0) for k in range(lv.n_tu)]
    items += [(lv.joint_arr[k].pred, c, lv.joint_arr[k].outOff, c) for k in range(lv.n_joint) for c in (0, 1)]
    dj = (DistJob * len(items))()
    for k, (p, c, out_off, buf) in enumerate(items):
        b = lv.block_of_pred(p)
        dj[k] = DistJob(b["org_off"][c], buf * len(got["reco"]) + out_off, b["org_stride"], b["w"], b["w"], b["h"], 0, lib.DIST_SSE)
    d_org, d_cur = ctx.to_device(lv.plane), ctx.to_device(np.concatenate([got["reco"], got["recoCr"]]))
    d_dj, d_out = ctx.to_device(struct_array_to_numpy(dj)), ctx.alloc(8 * len(items))
    ctx.dist_batch(d_org.ptr, d_cur.ptr, d_dj.ptr, len(items), d_out.ptr)
    ctx.sync()
    sse = d_out.to_host(np.uint64, shape=(-1,))
    assert np.array_equal(sse[:lv.n_tu], got["results"]["sse"][:lv.n_tu])
    assert np.array_equal(sse[lv.n_tu:].reshape(-1, 2), np.stack([got["jres"]["sseCb"][:lv.n_joint], got["jres"]["sseCr"][:lv.n_joint]], axis=1))
    for b in (d_org, d_cur, d_dj, d_out):
        b.free()


CLIP_SIZES = [(4, 4), (8, 8), (16, 16), (8, 4), (4, 16), (8, 8), (4, 4), (16, 16)]


def clip_level():
    """10 bits.  The lines of a block are flat, 120 from one end of the sample range (the ends alternate block by block), so every prediction is that flat value; the
    originals lie within 3 of either end, alternating sample by sample; base QPs 38 .. 47: the reconstructed residual overshoots and the clip acts at both ends.
    The last two blocks have their originals within 3 of the end their lines are near and lines 5 from it: a residual that quantises to nothing."""
    rng = np.random.default_rng(11)
    shapes = [(w, h, 10, "const", "full", k & 1 == 1, False, [(0, 1, 50, 18)[k % 4], 67 + k % 3]) for k, (w, h) in enumerate(CLIP_SIZES)]
    blocks = [cu.make_block(rng, w, h, bd, kind, cls, coloc=coloc, first_row=first, modes=modes, k=k) for k, (w, h, bd, kind, cls, coloc, first, modes) in enumerate(shapes)]
    for k, b in enumerate(blocks):
        quiet, hi = k >= len(blocks) - 2, k & 1
        v = (5 if quiet else 120) if not hi else 1023 - (5 if quiet else 120)
        b["lines"] = [(np.full(2 * b["w"] + 1, v, np.int16), np.full(2 * b["h"] + 1, v, np.int16)) for _ in (0, 1)]
        b["kind"], b["quiet"], b["hi"] = "flat", quiet, hi
    plane = cu.place_orgs(rng, blocks)
    for b in blocks:
        for c in (0, 1):
            (x, y), shp = b["org_xy"][c], (b["h"], b["w"])
            end = np.full(shp, b["hi"]) if b["quiet"] else rng.integers(0, 2, shp)
            plane[y:y + b["h"], x:x + b["w"]] = np.where(end == 1, 1023 - rng.integers(0, 4, shp), rng.integers(0, 4, shp))

    def cand(p, b):
        qp = lambda k: 38 + (3 * p + 2 * k) % 10      # noqa: E731
        adj = ccu.ADJS[(p + 1) % 5] if b["quiet"] else ccu.ADJS[p % 5]
        return ([(c, t, qp(k), k & 1, adj) for k, (c, t) in enumerate([(0, 0), (1, 0), (p & 1, 1)])],
                [(m, (p + m) & 1, int(m == 1 + p % 3), qp(m), m & 1, adj) for m in (1, 2, 3)])

    preds = [i for i, b in enumerate(blocks) for _ in b["modes"]]
    singles, joints = [], []
    for p, i in enumerate(preds):
        s, j = cand(p, blocks[i])
        singles += [(p,) + c for c in s]
        joints += [(p,) + c for c in j]
    return ccu.Level(blocks, plane, singles, joints)


def test_clip_case(ctx):
    lv = clip_level()
    # the restatements and the oracle alone say that these inputs clip at both ends and separate the two SSEs
    os_, oj = [lv.oracle_single(k) for k in range(lv.n_tu)], [lv.oracle_joint(k) for k in range(lv.n_joint)]
    raws = [e["raw"] for e in os_] + [r for e in oj for r in e["raw"]]
    assert sum(int((r < 0).sum()) for r in raws) > 0 and sum(int((r > 1023).sum()) for r in raws) > 0
    assert 2 * sum(e["result"][0] != e["result"][1] for e in os_) >= lv.n_tu
    assert 2 * sum(e["result"][0] != e["result"][2] or e["result"][1] != e["result"][3] for e in oj) >= lv.n_joint
    assert {e["result"][3] > 0 for e in os_} == {False, True} and {e["result"][6] > 0 for e in oj} == {False, True}
    # an uncoded job with an adj: the reconstruction is the clipped prediction (the reference's uiAbsSum > 0 guard on the inverse scaling changes nothing)
    quiet = [k for k in range(lv.n_tu) if os_[k]["result"][3] == 0 and lv.tu_arr[k].chromaAdj]
    quiet_j = [k for k in range(lv.n_joint) if oj[k]["result"][6] == 0 and lv.joint_arr[k].chromaAdj]
    assert quiet and quiet_j
    for k in quiet:
        assert np.array_equal(os_[k]["reco"], os_[k]["pred"])
    exp = lv.expect(ctx)
    assert exp["clipped"][0] > 0 and exp["clipped"][1] > 0
    got = lv.run(ctx)
    lv.check(got, exp)
    for k in range(lv.n_tu):
        lv.check_oracle_single(got, k)
    for k in range(lv.n_joint):
        lv.check_oracle_joint(got, k)
    for k in quiet:
        t = lv.tu_arr[k]
        i, cb, cr = lv.preds[t.pred]
        n, po = lv.blocks[i]["w"] * lv.blocks[i]["h"], cr if t.component else cb
        assert np.array_equal(got["reco"][t.outOff:t.outOff + n], got["pred"][po:po + n])
    for k in quiet_j:
        t = lv.joint_arr[k]
        i, cb, cr = lv.preds[t.pred]
        n = lv.blocks[i]["w"] * lv.blocks[i]["h"]
        assert np.array_equal(got["reco"][t.outOff:t.outOff + n], got["pred"][cb:cb + n]) and np.array_equal(got["recoCr"][t.outOff:t.outOff + n], got["pred"][cr:cr + n])


def test_table_forms(ctx, levels):
    base = levels["small-ts"]
    exp = base.expect(ctx)
    # no levels buffer: everything else as before
    base.check(base.run(ctx, levels=False), exp, levels=False)
    # the prediction + residual pass alone
    got = base.run(ctx, n_tu=0, n_joint=0)
    assert got["status"] == lib.OK and np.array_equal(got["pred"], exp["pred"]) and np.array_equal(got["resi"], exp["resi"])
    assert all((got[k].view(np.uint8) == ccu.FILL).all() for k in ("levels", "reco", "recoCr", "results", "jres"))
    # only single jobs; only joint jobs
    only = ccu.Level(base.blocks, base.plane, base.singles, [])
    only.check(only.run(ctx), only.expect(ctx))
    only = ccu.Level(base.blocks, base.plane, [], base.joints)
    only.check(only.run(ctx), only.expect(ctx))
    # all three tables shuffled: candidates of one prediction scattered through the arrays, the predictions of one block through theirs
    rng = np.random.default_rng(9)
    shapes, cand = CASES["small-ts"]
    s = ccu.make_level(np.random.default_rng(506), shapes, cand, order=(rng.permutation(base.n_tu), rng.permutation(base.n_joint)), job_order=rng.permutation(base.n_pred))
    assert (s.n_tu, s.n_joint) == (base.n_tu, base.n_joint) and sum(s.job_arr[k].block != s.job_arr[k + 1].block for k in range(s.n_pred - 1)) > s.n_pred // 2
    s.check(s.run(ctx), s.expect(ctx))
    # six jobs on one prediction, and predictions that no job names
    p = next(k for k in range(base.n_pred) if base.job_arr[k].mode >= 67)
    six = ccu.Level(base.blocks, base.plane, [(p, 0, 0, 27, 1, 3277), (p, 0, 1, 27, 0, 3277), (p, 1, 0, 30, 1, 0)], [(p, 1, 0, 0, 27, 0, 3277), (p, 2, 1, 1, 27, 1, 5000), (p, 3, 0, 0, 30, 0, 0)])
    six.check(six.run(ctx), six.expect(ctx))
    # no LM job: the luma plane is not needed; with one LM job it is
    blocks = [dict(b, modes=[m for m in b["modes"] if m < 67]) for b in base.blocks]
    no_lm = ccu.Level(blocks, base.plane, [(k, k & 1, 0, 30, 0, 2048) for k in range(0, 8)], [(k, 1 + k % 3, 0, 0, 30, 0, 2048) for k in range(4)])
    assert all(no_lm.job_arr[k].mode < 67 for k in range(no_lm.n_pred))
    no_lm.check(no_lm.run(ctx, luma=False), no_lm.expect(ctx))
    blocks[2] = dict(blocks[2], modes=blocks[2]["modes"] + [68])
    one_lm = ccu.Level(blocks, base.plane, no_lm.singles, no_lm.joints)
    got = one_lm.run(ctx, luma=False)
    assert got["status"] == lib.E_INVALID and one_lm.untouched(got)
    one_lm.check(one_lm.run(ctx), one_lm.expect(ctx))


@pytest.mark.parametrize("name,defect", ccu.DEFECTS, ids=[n for n, _ in ccu.DEFECTS])
def test_a_malformed_table_launches_nothing(ctx, name, defect):
    lv = ccu.base_level()
    defect(lv)
    got = lv.run(ctx)
    assert got["status"] == lib.E_INVALID and lv.untouched(got)


def test_the_base_table_of_the_rejections_runs(ctx):
    lv = ccu.base_level()
    lv.check(lv.run(ctx), lv.expect(ctx))


def test_null_pointers_and_negative_counts(ctx):
    """a well-formed table throughout: the NULL pointer or the negative count is the only defect, and nothing is written"""
    lv = ccu.base_level()
    # ref, luma, org, blocks, numBlocks, jobs, nPred, single jobs, nTu, joint jobs, nJoint, pred, resi, reco, recoCr, results, joint results, levels
    good, ins, outs = lv.device_args(ctx)
    assert all(good) and len(good) == 18

    def untouched():
        ctx.sync()
        return all((b.to_host(np.uint8, shape=(-1,)) == ccu.FILL).all() for b in outs)

    for k in (0, 1, 2, 3, 5, 7, 9, 11, 12, 13, 14, 15, 16):
        bad = list(good)
        bad[k] = None
        with pytest.raises(VtmHipError) as e:
            ctx.intra_chroma_chain_batch(*bad)
        assert e.value.status == lib.E_INVALID and untouched(), k
    for k in (4, 6, 8, 10):
        bad = list(good)
        bad[k] = -1
        with pytest.raises(VtmHipError) as e:
            ctx.intra_chroma_chain_batch(*bad)
        assert e.value.status == lib.E_INVALID and untouched(), k
    # the pointers a call does not need may be NULL: no tables at all; no jobs of either kind; no joint jobs
    ctx.intra_chroma_chain_batch(None, None, None, None, 0, None, 0, None, 0, None, 0, None, None, None, None, None, None)
    assert untouched()
    ctx.intra_chroma_chain_batch(*good[:7], None, 0, None, 0, good[11], good[12], None, None, None, None)
    assert not untouched()
    ctx.intra_chroma_chain_batch(*good[:9], None, 0, *good[11:14], None, good[15], None)
    ctx.intra_chroma_chain_batch(*good)                 # and the same arguments unharmed are accepted
    ctx.sync()
    for b in ins + outs:
        b.free()
