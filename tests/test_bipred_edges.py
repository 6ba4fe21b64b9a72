"""BDOF / DMVR at their decision edges, CPU side: the census of the edge tables (bipred_edge_util) on the oracle's own trace, and the oracle against the
reference on the same tables.  The GPU side is test_gpu_bipred_edges.py.

The census is a set of CONDITIONS on constructed inputs, not a measurement: every job is built so that the reference's arithmetic alone puts it into its
class, classify() asserts that per job, and the counts below only make sure no class got lost.

Thresholds.  dx * dy - 1, dx * dy, 2 * dx * dy - 1 and 2 * dx * dy are hit exactly at 10 and 12 bits.  At 8 bits every cost is a multiple of 4, so an
off-centre cost is 4k and a discounted centre 3k; the tables then use the nearest reachable value on each side:
    dx * dy = 128:  centre 126 | 129 and 255 | 258,  off-centre winner 252 | 256
    dx * dy = 256:  centre 255 | 258 and 510 | 513,  off-centre winner 508 | 512
so the only cells left out are the 8-bit `exact_*` ones whose value is no multiple of 3 (centre) or 4 (winner)."""
import ctypes as C

import numpy as np
import pytest

import bipred_edge_util as U
import oracle_lib as ol

SUBPU = [(8, 16, False), (16, 8, False), (16, 16, False)]
NEED = {
    "thr": ["centre_T-", "centre_T", "centre_2T-", "centre_2T", "winner_2T-", "winner_2T", "edge_skip", "centre_T_moves"],
    "tie": ["tie_rows", "tie_same_row", "plus8_h", "plus8_v", "minus8_h", "minus8_v", "zero_h", "zero_v", "div+_h", "div-_h", "div+_v", "div-_v",
            "disc_stay", "disc_move", "bio_off_by_winner_only"],
    "clip": ["clip_changes_phase", "plus8_h", "plus8_v", "div+_h", "div-_h", "div+_v", "div-_v", "edge_skip"],
}
EXACT = {"exact_centre_T-": (-1, 1, 3), "exact_centre_T": (0, 1, 3), "exact_centre_T_moves": (0, 1, 3), "exact_centre_2T-": (-1, 2, 3), "exact_centre_2T": (0, 2, 3),
         "exact_winner_2T-": (-1, 2, 4), "exact_winner_2T": (0, 2, 4)}      # class -> (offset, multiple of dx * dy, what an 8-bit cost of the kind is a multiple of)


@pytest.mark.parametrize("bd", U.DEPTHS)
@pytest.mark.parametrize("name", U.DMVR_TABLES)
def test_dmvr_census(name, bd):
    tab = U.dmvr_table(name, bd)
    census = U.dmvr_census(tab)      # asserts every job's own class
    assert 60 <= tab.n <= 240 and abs(2 * sum(j["bio"] for j in tab.jobs) - tab.n) <= 1
    assert max(max(j["w"], j["h"]) for j in tab.jobs) <= 32
    for cell in SUBPU:
        for cls in NEED[name]:
            assert census[cell].get(cls, 0) >= 4, (name, bd, cell, cls, census[cell])
        if name == "thr":
            for cls, (d, m, mult) in EXACT.items():
                value = m * cell[0] * cell[1] + d
                if bd == 8 and value % mult:
                    assert cls not in census[cell]      # left out: not a cost an 8-bit sub-PU of this shape can have (module docstring)
                    continue
                assert census[cell].get(cls, 0) >= 4, (bd, cell, cls, census[cell])
    if name != "clip":      # the 32 x 32 PU: four sub-PUs in four classes
        assert sum(census[(16, 16, True)].values()) > 0 and sum(1 for j in tab.jobs if j["nsub"] == 4) == 1


@pytest.mark.parametrize("bd", U.DEPTHS)
def test_dmvr_tables_move_chroma_every_way(bd):
    """The vector differences the chroma kernel is fed: unmoved sub-PUs and moves by +-8, +-24 and +-32 on either axis."""
    seen = set()
    for name in U.DMVR_TABLES:
        tab = U.dmvr_table(name, bd)
        for k, j in enumerate(tab.jobs):
            for s in range(j["nsub"]):
                seen.update((axis, int(v)) for axis, v in enumerate(tab.expect()["mvd"][k, s]))
    for axis in (0, 1):
        for v in (0, 8, -8, 24, 32, -32):
            assert (axis, v) in seen, (bd, axis, v, sorted(seen))
        assert (axis, -20) in seen and (axis, -12) in seen, (bd, axis)      # -24 cannot occur: -8 is the centre's alone and a winner at -32 skips the surface


@pytest.mark.parametrize("bd", U.DEPTHS)
def test_bdof_census(bd):
    tab = U.bdof_table(bd)
    counts = tab.expect()["counts"]
    assert 100 <= tab.n <= 240
    for (w, h) in U.SHAPES + ((32, 32),):
        total = ol.BdofTrace()
        for g in ("diag", "anti", "close", "cols", "rows", "low", "high"):
            total.add(counts[(w, h, g)])
        if (w, h) != (32, 32):
            for name, v in total.as_dict().items():
                assert v >= 4, (bd, w, h, name, total.as_dict())
        c = counts[(w, h, "close")]
        assert 2 * (c.tmpxLow + c.tmpxHigh + c.tmpyLow + c.tmpyHigh) <= c.units, (bd, w, h, c.as_dict())      # mostly unclamped
        d, a = counts[(w, h, "diag")], counts[(w, h, "anti")]
        assert 2 * d.signGe4096 >= d.units and 2 * a.signLtM4096 >= a.units, (bd, w, h, d.as_dict(), a.as_dict())
        assert counts[(w, h, "cols")].absGYZero >= 4 and counts[(w, h, "rows")].absGXZero >= 4, (bd, w, h)
        assert counts[(w, h, "low")].clipZero >= 4 and counts[(w, h, "high")].clipMax >= 4, (bd, w, h)


def test_tables_draw_nothing(monkeypatch):
    """VTM_TEST_SEED_OFFSET shifts every default_rng seed; the builders must not own one, or a soak run could move a job out of its class."""
    def no_rng(*a, **k):
        raise AssertionError("the edge tables must not draw")
    monkeypatch.setattr(np.random, "default_rng", no_rng)
    U.DmvrTable("tie", 10, U.tie_specs(10))
    U.DmvrTable("thr", 8, U.threshold_specs(8))
    U.DmvrTable("clip", 12, U.clip_specs(12))
    U.BdofTable(12)


def test_trace_variants_change_nothing(oracle):
    """vo_dmvr_pu / vo_bdof_pu (what every other test and the benchmark call) give what the trace variants give."""
    tab = U.dmvr_table("tie", 10)
    exp = tab.expect()
    for k, j in enumerate(tab.jobs):
        e, mvd = np.zeros((j["h"], j["w"]), np.int16), np.zeros(2 * j["nsub"], np.int32)
        oracle.vo_dmvr_pu(tab.luma_origin(k, 0), tab.luma_origin(k, 1), j["S"], U.PIC_W, U.PIC_H, U.CTU, j["x"], j["y"], j["w"], j["h"], *j["mv"], 10, j["bio"],
                          ol.P(e), j["w"], ol.P(mvd))
        assert np.array_equal(e, exp["pred"][k]) and np.array_equal(mvd.reshape(-1, 2), exp["mvd"][k, :j["nsub"]]), k
    bt = U.bdof_table(10)
    for k, j in enumerate(bt.jobs):
        e = np.zeros((j["h"], j["w"]), np.int16)
        at = [C.c_void_p(bt.refs.ctypes.data + 2 * j["off"][l]) for l in range(2)]
        oracle.vo_bdof_pu(at[0], j["S"], at[1], j["S"], j["w"], j["h"], *j["mv"], 10, ol.P(e), j["w"])
        assert np.array_equal(e, bt.expect()["pred"][k]), k


# ------------------------------------------------------------------------------------------------ the oracle against the reference, on the same tables
@pytest.mark.ref
@pytest.mark.parametrize("bd", U.DEPTHS)
@pytest.mark.parametrize("name", U.DMVR_TABLES)
def test_dmvr_edges_equal_reference(reflib, name, bd):
    """ref_dmvr_pu (luma rig) and ref_dmvr_pu420 (luma + both chroma planes) vs vo_dmvr_pu / vo_dmvr_chroma: predictions and vector differences bit-exact."""
    tab = U.dmvr_table(name, bd)
    exp = tab.expect()
    for k, j in enumerate(tab.jobs):
        w, h, ns = j["w"], j["h"], j["nsub"]
        a, ma = np.zeros((h, w), np.int16), np.zeros(2 * ns, np.int32)
        reflib.ref_dmvr_pu(tab.luma_origin(k, 0), tab.luma_origin(k, 1), j["S"], U.PIC_W, U.PIC_H, U.CTU, j["x"], j["y"], w, h, *j["mv"], bd, j["bio"], ol.P(a), w,
                           ol.P(ma))
        assert np.array_equal(ma.reshape(-1, 2), exp["mvd"][k, :ns]), (name, bd, k, j["label"], ma, exp["mvd"][k, :ns])
        assert np.array_equal(a, exp["pred"][k]), (name, bd, k, j["label"])
        planes = ((C.c_void_p * 3) * 2)()
        for l in range(2):
            planes[l][0] = tab.luma_origin(k, l).value
            for c in range(2):
                planes[l][1 + c] = tab.chroma_origin(k, l, c).value
        d = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
        dp = (C.c_void_p * 3)(*[x.ctypes.data for x in d])
        mb = np.zeros(2 * ns, np.int32)
        reflib.ref_dmvr_pu420(planes, j["S"], j["Sc"], U.PIC_W, U.PIC_H, U.CTU, j["x"], j["y"], w, h, *j["mv"], bd, j["bio"], dp, w, w // 2, ol.P(mb))
        assert np.array_equal(mb, ma) and np.array_equal(d[0], exp["pred"][k]), (name, bd, k, j["label"])
        for c in range(2):
            assert np.array_equal(d[1 + c], exp["cpred"][k][c]), (name, bd, k, c, j["label"], exp["mvd"][k, :ns])


@pytest.mark.ref
@pytest.mark.parametrize("bd", U.DEPTHS)
def test_bdof_edges_equal_reference(reflib, bd):
    """ref_bdof_pu with the scalar and with the x86 buffer operations vs vo_bdof_pu."""
    tab = U.bdof_table(bd)
    exp = tab.expect()
    for k, j in enumerate(tab.jobs):
        w, h = j["w"], j["h"]
        org = [C.c_void_p(tab.refs.ctypes.data + 2 * (j["off"][l] - (j["y"] * j["S"] + j["x"]))) for l in range(2)]
        for simd in (0, 1):
            a = np.zeros((h, w), np.int16)
            reflib.ref_bdof_pu(simd, org[0], org[1], j["S"], U.PIC_W, U.PIC_H, j["x"], j["y"], w, h, *j["mv"], bd, ol.P(a), w)
            assert np.array_equal(a, exp["pred"][k]), (bd, k, simd, j["group"], j["mv"])
