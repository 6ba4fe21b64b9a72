"""CPU checks of the chroma intra rules: the numpy restatement (tests/cclm_util.py) against hand-computed cases and its own invariants, vtmhip_cclm_params (the
C++ rules of vtm_amd/csrc/cclm_rules.hpp run on host pointers) against the restatement over every block size x availability class x plane kind, and the struct
sizes.  The parity tests skip without a built library, as tests/test_intra.py does."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

import cclm_util as cu
import intra_util as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_lib = pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "vtm_amd", "libvtmhip.so")), reason="libvtmhip.so not built")


def test_significand_table_is_the_closed_form():
    assert cu.DIV_SIG_TABLE[0] == 0
    assert cu.DIV_SIG_TABLE[1:] == [(2 * 256 + 16 + n) // (2 * (16 + n)) - 8 for n in range(1, 16)]     # round(256 / (16 + n)) - 8


def test_pairs_by_hand():
    assert cu.pairs_to_params([0] * 4, [0] * 4, 0, 10) == (0, 512, 0)
    # two pairs: diff 64 -> x 6, v 8; diffC 32 -> y 6: a = (256 + 32) >> 6 = 4, shift 3, b = 50 - (400 >> 3)
    assert cu.pairs_to_params([100, 164], [50, 82], 2, 10) == (4, 0, 3) == cu.pairs_to_params([164, 100], [82, 50], 2, 10)
    # four pairs: (10, 20) and (110, 120) are averaged; diff 100 -> normDiff 9, v 10, x 7; diffC 280 -> y 9: a = 3056 >> 9 = 5, shift 1
    assert cu.pairs_to_params([120, 10, 20, 110], [400, 100, 120, 380], 4, 10) == (5, 110 - ((5 * 15) >> 1), 1)
    assert cu.pairs_to_params([77] * 4, [1, 2, 3, 4], 4, 8) == (0, 2, 0)
    assert cu.pairs_to_params([500, 501, 500, 501], [0, 4095, 0, 4095], 4, 12) == (15, -3750, 1)
    assert cu.pairs_to_params([500, 501, 500, 501], [4095, 0, 4095, 0], 4, 12) == (-15, 4095 + 3750, 1)
    assert cu.pairs_to_params([10, 900, 10, 900], [33] * 4, 4, 10)[:2] == (0, 33)


def test_downsampling_by_hand():
    """a plane of x + 10 y: every filter is an average with weights summing to a power of two, so the result is the filter's centre of mass"""
    rng = np.random.default_rng(0)
    for coloc in (False, True):
        b = cu.make_block(rng, 4, 4, 10, "const", "full", coloc=coloc, modes=[])
        x0, y0 = b["lxy"]
        ys, xs = np.mgrid[0:b["plane"].shape[0], 0:b["plane"].shape[1]]
        b["plane"] = ((xs - x0) + 10 * (ys - y0) + 100).astype(np.int16)
        inner, top, left = cu.downsample(b, True)
        # collocated: the cross centred on (2i, 2j); default: centred between rows 2j and 2j + 1: + 5, and (s + 4) >> 3 of 8 * centre + 40 = centre + 5
        cy = 0 if coloc else 5
        assert inner[1, 2] == 100 + 4 + 20 + cy and inner[0, 0] == 100 + cy
        assert top[3] == 100 + 6 - 20 + cy and top.size == 8 and left[2] == 100 - 2 + 40 + cy and left.size == 8
        b["first_row"] = True
        assert cu.downsample(b, False)[1][3] == 100 + 6 - 10 and cu.downsample(b, False)[1].size == 4
    # without neighbours the padded taps repeat the centre column / row
    b = cu.make_block(rng, 4, 4, 10, "const", "none", coloc=True, modes=[])
    x0, y0 = b["lxy"]
    b["plane"][y0:y0 + 8, x0:x0 + 8] = np.arange(64).reshape(8, 8) * 3
    p = b["plane"].astype(int)
    inner, top, left = cu.downsample(b, True)
    assert top is None and left is None
    assert inner[0, 0] == (4 + 6 * p[y0, x0] + p[y0, x0 + 1] + p[y0 + 1, x0]) >> 3
    assert inner[0, 1] == (4 + 5 * p[y0, x0 + 2] + p[y0, x0 + 1] + p[y0, x0 + 3] + p[y0 + 1, x0 + 2]) >> 3


def test_chroma_regular_modes_differ_from_luma_only_where_the_rules_say():
    """no reference filter, no smoothing taps, two taps instead of the cubic: integer slopes, DC and small planar blocks agree with the luma restatement"""
    rng = np.random.default_rng(4)
    for w, h in cu.SHAPES10:
        top, left = iu.make_lines(rng, w, h, 0, 10, "random")
        for mode in range(67):
            pl, pc = iu.params(w, h, mode, 0), cu.chroma_params(w, h, mode)
            assert {k: pc[k] for k in pc if k not in ("refFilterFlag", "interpolationFlag")} == {k: pl[k] for k in pl if k not in ("refFilterFlag", "interpolationFlag")}
            got = cu.predict_regular(top, left, w, h, mode, 10)
            assert got.min() >= 0 and got.max() <= 1023
            same_rule = not pl["refFilterFlag"] and (mode < 2 or not (abs(pl["intraPredAngle"]) & 31))
            if same_rule:
                assert np.array_equal(got, iu.predict(top, left, w, h, mode, 0, 10)), (w, h, mode)
    # a fractional slope by hand: mode 51 on 4x4 (angle 1): row y takes top[x + 1] + ((y + 1) * (top[x + 2] - top[x + 1]) + 16 >> 5), then the PDPC column
    top, left = np.arange(9) * 64, np.full(9, 0)
    left[0] = top[0]
    p = cu.chroma_params(4, 4, 51)
    assert p["intraPredAngle"] == 1 and p["applyPDPC"] == 0      # angularScale < 0 for the steepest slope
    got = cu.predict_regular(top, left, 4, 4, 51, 10)
    assert got[0].tolist() == [64 + 2, 128 + 2, 192 + 2, 256 + 2] and got[3, 0] == 64 + ((4 * 64 + 16) >> 5)


GOLDEN = os.path.join(ROOT, "tests", "golden", "cclm.npz")


@pytest.fixture(scope="module")
def golden():
    return list(cu.golden_cases(GOLDEN))


def _ds_equal(got, rec, w, h):
    """the restatement's (inner, top, left) against the recorded buffer: equal where the reference filled it, GOLDEN_UNSET beyond"""
    inner, top, left = got
    assert np.array_equal(inner, rec[0])
    for g, r, n in ((top, rec[1], 2 * w), (left, rec[2], 2 * h)):
        k = 0 if g is None else g.size
        assert (k == 0 or np.array_equal(g, r[:k])) and (r[k:] == cu.GOLDEN_UNSET).all() and r.size == n


def test_restatement_equals_the_recorded_reference(golden):
    """sample for sample and parameter for parameter: the down-sampled luma of both extents, (a, b, shift) of 3 modes x 2 components, the LM and regular predictions"""
    assert len(golden) == 140 and {(b["w"], b["h"]) for b, *_ in golden} == set(cu.SHAPES10) and {b["bd"] for b, *_ in golden} == {8, 10, 12}
    assert {(b["above"], b["left"]) for b, *_ in golden} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(b["first_row"] for b, *_ in golden) and {b["coloc"] for b, *_ in golden} == {False, True}
    for b, ds_lm, ds_md, par, p_lm, modes, p_rg in golden:
        w, h = b["w"], b["h"]
        lm, md = cu.downsample(b, False), cu.downsample(b, True)
        _ds_equal(lm, ds_lm, w, h)
        _ds_equal(md, ds_md, w, h)
        for mode in cu.ALL_LM:
            for c in (0, 1):
                assert tuple(cu.lm_params(b, c, mode, md if mode != cu.LM else lm)) == tuple(int(v) for v in par[mode - cu.LM, c]), (w, h, mode, c)
            assert np.array_equal(cu.predict(b, mode), p_lm[mode - cu.LM]), (w, h, mode)
        for k, mode in enumerate(modes):
            assert np.array_equal(cu.predict(b, mode), p_rg[k]), (w, h, mode)


@needs_lib
def test_cclm_params_equal_the_recorded_reference(golden):
    from vtm_amd import device
    batch = cu.Batch([b for b, *_ in golden])
    for b, _, _, par, _, _, _ in golden:
        for mode in cu.ALL_LM:
            for c in (0, 1):
                assert device.cclm_params(b, batch.ref_buf, batch.luma_buf, c, mode) == tuple(int(v) for v in par[mode - cu.LM, c])


@pytest.fixture(scope="module")
def grid():
    rng, blocks, k = np.random.default_rng(2025), [], 0
    for w, h in cu.SHAPES10:
        for cls in cu.AVAIL_CLASSES:
            for kind in ("random", "alt", "const", "swing"):
                for coloc in (False, True):
                    blocks.append(cu.make_block(rng, w, h, (8, 10, 12)[k % 3], kind, cls, coloc=coloc, first_row=k % 5 == 0, modes=[], k=k))
                    k += 1
    return blocks, cu.Batch(blocks)


def test_restatement_reaches_every_branch(grid):
    blocks, _ = grid
    seen = collections.Counter()
    for b in blocks:
        ds = {m: cu.downsample(b, m) for m in (False, True)}
        for mode in cu.ALL_LM:
            for c in (0, 1):
                info = {}
                cu.lm_params(b, c, mode, ds[mode != cu.LM], info)
                for key, v in info.items():
                    seen[(key, int(np.sign(v))) if key in ("clamp", "a") else key] += 1
    for key in ("none", "diff0", ("clamp", 1), ("clamp", -1), ("a", -1), ("a", 1), "ar_clamp", "bl_clamp"):
        assert seen[key] >= 5, (key, seen)


@needs_lib
def test_struct_sizes():
    from vtm_amd import lib
    L = lib.load()
    assert [L.vtmhip_intra_chroma_struct_size(i) for i in range(4)] == [64, 24, 12, -1]
    assert [C.sizeof(s) for s in (lib.IntraChromaBlock, lib.IntraChromaJob, lib.CclmModel)] == [64, 24, 12]
    assert L.vtmhip_intra_struct_size(3) == -1            # the luma list is unchanged


@needs_lib
def test_cclm_params_parity(grid):
    """vtmhip_cclm_params == the restatement for every block x component x LM mode; the poisoned planes show that the C++ closed form reads nothing the loops do not"""
    from vtm_amd import device
    blocks, batch = grid
    n = 0
    for b in blocks:
        ds = {m: cu.downsample(b, m) for m in (False, True)}
        for mode in cu.ALL_LM:
            for c in (0, 1):
                exp = cu.lm_params(b, c, mode, ds[mode != cu.LM])
                assert device.cclm_params(b, batch.ref_buf, batch.luma_buf, c, mode) == tuple(int(v) for v in exp), (b["w"], b["h"], b["above"], b["left"], mode, c)
                n += 1
    assert n == len(blocks) * 6


@needs_lib
def test_cclm_params_rejects_malformed_input(grid):
    from vtm_amd import device, lib
    blocks, batch = grid
    good = next(b for b in blocks if b["ar"] and b["bl"])
    for field, v in (("w", 2), ("h", 64), ("bd", 13), ("ar", 3), ("bl", good["h"] + 2), ("above", False)):
        bad = dict(good)
        bad[field] = v
        with pytest.raises(lib.VtmHipError) as e:
            device.cclm_params(bad, batch.ref_buf, batch.luma_buf, 0, 67)
        assert e.value.status == lib.E_INVALID
    for comp, mode in ((2, 67), (-1, 67), (0, 66), (0, 70)):
        with pytest.raises(lib.VtmHipError):
            device.cclm_params(good, batch.ref_buf, batch.luma_buf, comp, mode)
