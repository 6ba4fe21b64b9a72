"""GPU parity of vtmhip_intra_chain_batch_dev: prediction, residual, the fused chain, the clipped reconstruction and its SSE in one call.  Bit-exact, no tolerance.
The expectation is composed (intra_chain_util.Level.expect) from entries that are pinned to the reference -- vtmhip_intra_pred_batch_dev / vtmhip_mip_pred_batch_dev,
vtmhip_tu_chain_batch_dev with uniformSize == 0 on the uploaded residual -- with the residual, the reconstruction and the int64 SSE in numpy; the jobs on 4x4, 8x8 and
16x16 blocks are also checked against intra_util / mip_util and the oracle's xT -> quant -> dequant -> xIT, so one case per lane path rests on no device entry.
Every buffer is compared in full: the lines lie between runs of 0x7fff, the originals at odd offsets with stride 97, and every prediction and output block between
samples of fill that must stay."""
import ctypes as C

import numpy as np
import pytest

import intra_chain_util as icu
import mip_util as mu
from vtm_amd import lib
from vtm_amd.device import Context, struct_array_to_numpy
from vtm_amd.lib import DistJob, VtmHipError

pytestmark = pytest.mark.gpu

CANDS = [(lib.DCT2, lib.DCT2), (lib.DST7, lib.DST7), (lib.DCT8, lib.DST7), (lib.TRSKIP, lib.TRSKIP)]
QPS = (10, 27, 38, 51)
M7 = [0, 1, 2, 18, 34, 50, 66]


def tus_of(real_only=False):
    """every second prediction takes all its candidates (four share one prediction), the others 1 .. 4; a side of 64 takes DCT2 alone"""
    def f(p, b):
        c = CANDS[:1] if max(b["w"], b["h"]) > 32 else CANDS[:3] if real_only else CANDS
        n = len(c) if p % 2 == 0 else 1 + p % len(c)
        return [(th, tv, 45 if b["kind"] == "const" else QPS[(p + k) % 4], (p + k) & 1) for k, (th, tv) in enumerate(c[:n])]
    return f


# (w, h, multiRefIdx, bitDepth, regular modes, MIP (mode, transposed)[, kind]); what each case reaches: lanes per prediction job / chain path / lanes per finish job
CASES = {
    "4x4": (True, [(4, 4, 0, 8, M7, [(0, 0), (15, 1)]), (4, 4, 1, 10, [1, 2, 66], []), (4, 4, 2, 12, [18, 50], []), (4, 4, 0, 10, [0, 34], [(15, 0), (0, 1)]),
                   (4, 4, 0, 10, [0, 1, 50], [(3, 0)], "const")]),                                                  # 16 / one lane per TU / 16
    "small-mixed": (False, [(8, 4, 0, 10, [0, 1, 3, 18], [(0, 0), (7, 1)]), (4, 16, 1, 8, [1, 2, 60, 66], []), (8, 8, 2, 12, [34, 50], []),
                            (8, 8, 0, 10, M7, [(7, 0), (0, 1)]), (4, 16, 0, 12, [0, 50], [(7, 1)], "const")]),      # 16 / generic at 64 lanes / 16
    "8x8": (True, [(8, 8, 0, 10, M7, [(0, 0), (7, 1)]), (8, 8, 1, 8, [1, 18, 66], []), (8, 8, 2, 12, [2, 50], []), (8, 8, 0, 12, [0, 34], [(7, 0), (0, 1)]),
                   (8, 8, 0, 8, [1, 50], [(2, 1)], "const")]),                                                      # 16 / register-blocked / 16
    "medium": (False, [(16, 16, 0, 10, M7, [(0, 0), (5, 1)]), (32, 8, 1, 8, [1, 4, 18, 66], []), (8, 32, 2, 12, [2, 50, 62], []), (32, 8, 0, 12, [0, 34], [(5, 0), (0, 1)]),
                       (16, 16, 0, 8, [0, 66], [(1, 1)], "const")]),                                                # 64 / generic at 256 lanes / 64
    "large": (False, [(64, 64, 0, 10, [0, 1, 34], [(0, 0), (5, 1)]), (64, 16, 1, 8, [1, 5, 66], []), (64, 16, 2, 12, [18, 50], []), (64, 64, 0, 12, [2], [(5, 0), (0, 1)]),
                      (64, 16, 0, 10, [0, 50], [(2, 0)], "const")]),                                                # 256 / generic at 256 lanes / 64
    "bucketed": (False, [(s, s, m, bd, [1, 18, 34, 50, 66] + ([0] if m == 0 else [2]), [(0, 0), (5 if s > 8 else 7, 1)] if m == 0 else [])
                         for s, m, bd in ((8, 0, 10), (16, 1, 8), (32, 2, 12), (8, 2, 12), (16, 0, 10), (32, 0, 8), (8, 1, 8), (16, 2, 12), (32, 0, 10), (16, 0, 8), (8, 0, 12))]
                 + [(16, 16, 0, 10, [0, 50], [(1, 0)], "const")]),                                                  # 64 / bucketed by shape / 64
}


@pytest.fixture(scope="module")
def mctx(ctx):
    ctx.mip_set_tables(*mu.matrices())
    return ctx


@pytest.fixture(scope="module")
def levels():
    """the tables of every case, built once; Level.expect caches the composed expectation"""
    return {k: icu.make_level(np.random.default_rng(300 + i), shapes, tus_of(real)) for i, (k, (real, shapes)) in enumerate(CASES.items())}


def test_the_cases_reach_every_path(levels):
    L = lib.load()
    lanes, chain = {}, {}
    for k, lv in levels.items():
        _, mw, mh, uni = lv.tu_jobs()
        lanes[k] = L.vtmhip_intra_lanes_per_job(max(b["w"] * b["h"] for b in lv.blocks))
        chain[k] = ("lane" if mw * mh <= 32 else "blocked") if uni else "bucketed" if lv.n_tu >= 256 and min(mw, mh) >= 8 else "generic64" if mw * mh <= 256 else "generic256"
    assert lanes == {"4x4": 16, "small-mixed": 16, "8x8": 16, "medium": 64, "large": 256, "bucketed": 64}
    assert chain == {"4x4": "lane", "small-mixed": "generic64", "8x8": "blocked", "medium": "generic256", "large": "generic256", "bucketed": "bucketed"}
    allv = list(levels.values())
    assert {lv.blk_arr[i].bitDepth for lv in allv for i in range(len(lv.blocks))} == {8, 10, 12}
    assert {lv.blk_arr[i].multiRefIdx for lv in allv for i in range(len(lv.blocks))} == {0, 1, 2}
    assert {lv.intra_arr[k].mode for lv in allv for k in range(lv.n_intra)} >= set(M7) | {3, 4, 5, 60, 62}        # the last five: wide angles on flat / tall blocks
    assert {(lv.mip_arr[k].mode == 0, lv.mip_arr[k].transposed) for lv in allv for k in range(lv.n_mip)} == {(True, 0), (True, 1), (False, 0), (False, 1)}
    tu = [lv.tu_arr[k] for lv in allv for k in range(lv.n_tu)]
    assert {(t.typeHor, t.typeVer) for t in tu} == set(CANDS) and {t.isIRAP for t in tu} == {0, 1}
    assert any(t.typeHor == lib.TRSKIP and lv.block_of_tu(k)["w"] == 32 for lv in allv for k, t in enumerate(lv.tu_arr[j] for j in range(lv.n_tu)))
    for lv in allv:
        assert max(np.bincount([lv.tu_arr[k].pred for k in range(lv.n_tu)])) == (4 if any(t[1] == lib.TRSKIP for t in lv.tus) else 3 if lv.blocks[0]["w"] < 64 else 1)


@pytest.mark.parametrize("case", list(CASES))
def test_path_matrix(mctx, levels, case):
    lv = levels[case]
    exp = lv.expect(mctx)
    abs_sums = [r[3] for r in exp["results"]]
    assert min(abs_sums) == 0 and max(abs_sums) > 0                     # on the expected values: a cbf of 0 and of 1 both occur
    got = lv.run(mctx)
    assert got["status"] == lib.OK
    lv.check(got, exp)
    if case in ("4x4", "8x8", "medium"):                                 # without any device entry: the restatements and the oracle
        ks = [k for k in range(lv.n_tu) if lv.block_of_tu(k)["w"] == lv.block_of_tu(k)["h"]][:48]
        assert len(ks) >= 8 and {lv.tu_arr[k].pred >= lv.n_intra for k in ks} == {False, True}
        for k in ks:
            lv.check_oracle(got, k)


def test_sse_is_what_the_distortion_entry_gives(mctx, levels):
    lv = levels["small-mixed"]
    got = lv.run(mctx)
    dj = (DistJob * lv.n_tu)()
    for k in range(lv.n_tu):
        b = lv.block_of_tu(k)
        dj[k] = DistJob(b["org_off"], lv.tu_arr[k].outOff, b["org_stride"], b["w"], b["w"], b["h"], 0, lib.DIST_SSE)
    d_org, d_cur, d_dj, d_out = mctx.to_device(lv.plane), mctx.to_device(got["reco"]), mctx.to_device(struct_array_to_numpy(dj)), mctx.alloc(8 * lv.n_tu)
    mctx.dist_batch(d_org.ptr, d_cur.ptr, d_dj.ptr, lv.n_tu, d_out.ptr)
    mctx.sync()
    assert np.array_equal(d_out.to_host(np.uint64, shape=(-1,)), got["results"]["sse"][:lv.n_tu])
    for b in (d_org, d_cur, d_dj, d_out):
        b.free()


CLIP_SHAPES = [(8, 8, 0, 8, [0, 1, 18, 50], [(0, 0), (7, 1)]), (16, 16, 0, 10, [1, 34, 66], [(5, 0)]), (4, 4, 0, 12, [0, 2], [(15, 1)]), (16, 16, 1, 8, [2, 50], [])]


def clip_level():
    """originals within 3 of either end of the sample range, sample by sample, and coarse QPs: the reconstructed residual overshoots and the clip acts at both ends"""
    rng = np.random.default_rng(77)
    lv = icu.make_level(rng, CLIP_SHAPES, lambda p, b: [(th, tv, 44 + 3 * k, k & 1) for k, (th, tv) in enumerate(CANDS[:2 + p % 3])])
    for b in lv.blocks:
        (x, y), mx = b["org_xy"], (1 << b["bd"]) - 1
        lv.plane[y:y + b["h"], x:x + b["w"]] = np.where(rng.integers(0, 2, (b["h"], b["w"])) == 1, mx - rng.integers(0, 4, (b["h"], b["w"])), rng.integers(0, 4, (b["h"], b["w"])))
    return lv


def test_clip_case(mctx):
    lv = clip_level()
    # the restatements and the oracle alone say that this seed clips at both ends and separates the two SSEs
    ora = [lv.oracle_expect(k) for k in range(lv.n_tu)]
    assert sum(int((e["raw"] < 0).sum()) for e in ora) > 0 and sum(int((e["raw"] > (1 << lv.block_of_tu(k)["bd"]) - 1).sum()) for k, e in enumerate(ora)) > 0
    assert any(e["result"][0] != e["result"][1] for e in ora)
    exp = lv.expect(mctx)
    assert exp["clipped"][0] > 0 and exp["clipped"][1] > 0 and any(r[0] != r[1] for r in exp["results"])
    got = lv.run(mctx)
    lv.check(got, exp)
    for k in range(lv.n_tu):
        lv.check_oracle(got, k)


def test_table_forms(mctx, levels):
    base = levels["small-mixed"]
    exp = base.expect(mctx)
    # no levels buffer: everything else as before
    base.check(base.run(mctx, levels=False), exp, levels=False)
    # the prediction + residual pass alone
    got = base.run(mctx, n_tu=0)
    assert got["status"] == lib.OK and np.array_equal(got["pred"], exp["pred"]) and np.array_equal(got["resi"], exp["resi"])
    assert all((got[k].view(np.uint8) == icu.FILL).all() for k in ("levels", "reco", "results"))
    # the TU table shuffled: candidates of one prediction scattered through the array
    rng = np.random.default_rng(9)
    s = icu.Level(base.blocks, base.plane, base.tus, order=rng.permutation(base.n_tu))
    s.check(s.run(mctx), s.expect(mctx))
    # four candidates sharing one prediction, alone
    four = icu.Level(base.blocks, base.plane, [(3, th, tv, 27, 1) for th, tv in CANDS])
    four.check(four.run(mctx), four.expect(mctx))
    # an empty regular table (the MIP jobs alone), then an empty MIP table on a context that never saw the matrices
    blocks = [dict(b, modes=[]) for b in base.blocks if b["mip"]]
    only_mip = icu.Level(blocks, base.plane, [(p, lib.DCT2, lib.DCT2, 27, 0) for p in range(sum(len(b["mip"]) for b in blocks))])
    assert only_mip.n_intra == 0 and only_mip.n_mip >= 3
    only_mip.check(only_mip.run(mctx), only_mip.expect(mctx))
    blocks = [dict(b, mip=[]) for b in base.blocks]
    only_reg = icu.Level(blocks, base.plane, [(p, lib.DST7, lib.DCT8, 27, 0) for p in range(0, sum(len(b["modes"]) for b in blocks), 2)])
    assert only_reg.n_mip == 0
    fresh = Context(0)
    try:
        only_reg.check(only_reg.run(fresh), only_reg.expect(mctx))
        # MIP jobs before vtmhip_mip_set_tables: rejected, nothing written
        got = base.run(fresh)
        assert got["status"] == lib.E_INVALID and base.untouched(got)
    finally:
        fresh.close()


@pytest.mark.parametrize("name,defect", icu.DEFECTS, ids=[n for n, _ in icu.DEFECTS])
def test_a_malformed_table_launches_nothing(mctx, name, defect):
    lv = icu.base_level()
    defect(lv)
    got = lv.run(mctx)
    assert got["status"] == lib.E_INVALID and lv.untouched(got)


def test_the_base_table_of_the_rejections_runs(mctx):
    lv = icu.base_level()
    lv.check(lv.run(mctx), lv.expect(mctx))


def test_null_pointers_and_negative_counts(mctx):
    """a well-formed table throughout: the NULL pointer or the negative count is the only defect, and nothing is written"""
    lv = icu.base_level()
    good, ins, outs = lv.device_args(mctx)       # ref, org, blocks, numBlocks, intra jobs, nIntra, MIP jobs, nMip, TU jobs, nTu, pred, resi, reco, results, levels
    assert all(good) and len(good) == 15

    def untouched():
        mctx.sync()
        return all((b.to_host(np.uint8, shape=(-1,)) == icu.FILL).all() for b in outs)

    for k in (0, 1, 2, 4, 6, 8, 10, 11, 12, 13):
        bad = list(good)
        bad[k] = None
        with pytest.raises(VtmHipError) as e:
            mctx.intra_chain_batch(*bad)
        assert e.value.status == lib.E_INVALID and untouched(), k
    for k in (3, 5, 7, 9):
        bad = list(good)
        bad[k] = -1
        with pytest.raises(VtmHipError) as e:
            mctx.intra_chain_batch(*bad)
        assert e.value.status == lib.E_INVALID and untouched(), k
    # the pointers a call does not need may be NULL: no tables at all; no TU jobs (reconstruction, results and levels)
    mctx.intra_chain_batch(None, None, None, 0, None, 0, None, 0, None, 0, None, None, None, None)
    assert untouched()
    mctx.intra_chain_batch(*good[:8], None, 0, good[10], good[11], None, None, None)
    assert not untouched()
    mctx.intra_chain_batch(*good)                 # and the same arguments unharmed are accepted
    mctx.sync()
    for b in ins + outs:
        b.free()
