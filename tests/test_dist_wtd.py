"""CPU: the numpy restatement of the luma-level-weighted SSE (tests/wtd_util.py, reference CommonLib/RdCost.cpp:3055-3463) pinned to the real
reference -- per sample against RdCost::getWeightedMSE itself (`ref` marker) and per block against tests/golden/sse_wtd.npz -- and the ABI of the
DF_SSE_WTD family (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest

import wtd_util as wu
from vtm_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sse_wtd.npz")


@pytest.fixture(scope="module")
def refmse(reflib):
    return wu.RefWeightedMSE(reflib)


def _samples(rng, n, bd):
    mx = 1 << bd
    o = rng.integers(0, mx, n)
    c = rng.integers(0, mx, n)
    c[: n // 2] = np.clip(o[: n // 2] + rng.integers(-16, 17, n // 2), 0, mx - 1)   # small differences too
    return o, c, rng.integers(0, mx, n)


@pytest.mark.ref
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("signal", [wu.SDR, wu.PQ, wu.HLG])
def test_per_sample_rule_matches_reference(refmse, bd, signal):
    rng = np.random.default_rng(100 + bd * 3 + signal)
    lut, cw = wu.random_table(rng, bd), float(rng.uniform(0.25, 4.0))
    refmse.set_state(bd, signal, cw, lut)
    o, c, lv = _samples(rng, 600, bd)
    for comp in (0, 1, 2):
        l = o if comp == 0 else lv                      # the reference CHECKs orgLuma == org for luma
        got = [refmse.mse(comp, o[i], c[i], l[i]) for i in range(len(o))]
        exp = wu.mse_samples(comp, o, c, l, lut, signal, cw).astype(np.int64).astype(np.uint64)
        assert np.array_equal(np.array(got, np.uint64), exp), (comp, bd, signal)


@pytest.mark.ref
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_reference_pq_table_and_rule(refmse, bd):
    refmse.set_state(bd, wu.PQ, 1.0)                    # initLumaLevelToWeightTableReshape builds the PQ table
    tab = refmse.table(bd)
    assert np.allclose(tab, wu.pq_table(bd), rtol=1e-15, atol=0)                       # libm pow vs numpy: an ulp at most
    assert np.array_equal(wu.fixed_weights(tab), wu.fixed_weights(wu.pq_table(bd)))     # the weights the rule uses are identical
    rng = np.random.default_rng(7 + bd)
    o, c, lv = _samples(rng, 800, bd)
    for comp in (0, 1):
        l = o if comp == 0 else lv
        got = np.array([refmse.mse(comp, o[i], c[i], l[i]) for i in range(len(o))], np.uint64)
        assert np.array_equal(got, wu.mse_samples(comp, o, c, l, tab, wu.PQ, 1.0).astype(np.int64).astype(np.uint64))


@pytest.mark.ref
def test_large_weights_truncate_to_32_bits(refmse):
    """fixed * d * d >> 16 beyond 2^31: Intermediate_Int (int) keeps the low 32 bits, and a negative mse sign-extends into the sum."""
    bd = 12
    rng = np.random.default_rng(5)
    lut = rng.uniform(2000.0, 32767.0, 1 << bd)        # fixed weights up to just under 2^31
    refmse.set_state(bd, wu.SDR, 20000.0, lut)
    o, c, lv = _samples(rng, 1000, bd)
    c[:500] = np.where(o[:500] > 2048, 0, 4095)         # large differences
    wrapped = 0
    for comp in (0, 1):
        l = o if comp == 0 else lv
        got = np.array([refmse.mse(comp, o[i], c[i], l[i]) for i in range(len(o))], np.uint64)
        exp = wu.mse_samples(comp, o, c, l, lut, wu.SDR, 20000.0)
        assert np.array_equal(got, exp.astype(np.int64).astype(np.uint64))
        fx = wu.fixed_weights(lut)[l] if comp == 0 else wu.fixed_weights(20000.0)
        wrapped += int(np.sum(((fx * (o - c) ** 2 + 32768) >> 16) >= 2 ** 31))
    assert wrapped > 100                                # the case really exercises the truncation


def test_golden_reproduced_by_numpy_rule():
    z = np.load(GOLDEN)
    n = len(z["c_dist"])
    assert n > 100
    seen_w, seen_fmt = set(), set()
    for i in range(n):
        k, w, h, comp = int(z["c_set"][i]), int(z["c_w"][i]), int(z["c_h"][i]), int(z["c_comp"][i])
        sx, sy = int(z["c_csx"][i]), int(z["c_csy"][i])
        org = z["org"][z["c_org_off"][i]:][: w * h].reshape(h, w)
        cur = z["cur"][z["c_cur_off"][i]:][: w * h].reshape(h, w)
        ls = int(z["c_luma_stride"][i])
        luma = z["luma"][z["c_luma_off"][i]:][: (h << sy) * ls].reshape(-1, ls) if comp else None
        got = wu.sse_wtd(org, cur, comp, z["lut%d" % k], int(z["set_signal"][k]), float(z["set_chroma"][k]), luma, sx, sy)
        assert got == int(z["c_dist"][i]), i
        seen_w.add(w)
        seen_fmt.add((comp > 0, sx, sy))
    assert seen_w == {2, 4, 8, 16, 32, 64, 128, 6, 12, 24, 48}
    assert seen_fmt == {(False, 0, 0), (True, 1, 1), (True, 1, 0), (True, 0, 0)}
    assert set(z["set_bd"].tolist()) == {8, 10, 12} and set(z["set_signal"].tolist()) == {wu.SDR, wu.PQ}
    assert os.path.getsize(GOLDEN) <= 2 << 20


def test_wtd_job_layout_and_symbols():
    L = lib.load()
    assert C.sizeof(lib.WtdJob) == 48 and L.vtmhip_struct_size(33) == 48
    for s in ("vtmhip_set_luma_level_weights", "vtmhip_xGetSSE_WTD", "vtmhip_sse_wtd_batch_dev"):
        assert s in lib.exported_symbols() and hasattr(L, s)


def test_wtd_entries_fail_without_a_context():
    L = lib.load()
    lut = np.ones(1024)
    d = C.c_uint64()
    assert L.vtmhip_set_luma_level_weights(None, lut.ctypes.data, 10, 0, 1.0, None) == lib.E_INVALID
    o = np.zeros(16, np.int16)
    assert L.vtmhip_xGetSSE_WTD(None, o.ctypes.data, 4, o.ctypes.data, 4, 4, 4, 0, None, 0, 0, 0, C.byref(d)) == lib.E_INVALID
    assert L.vtmhip_sse_wtd_batch_dev(None, None, None, None, None, 1, None) == lib.E_INVALID
