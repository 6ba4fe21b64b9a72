"""CPU: intra sub-partitions (ISP) on the host -- the rules of vtm_amd/csrc/isp_rules.hpp through their host entries against tests/golden/isp.npz (recorded from the
reference's own members by tests/golden/gen_isp_golden.py) and against the restatement of isp_util; the oracle's transforms at the TU shapes only ISP has against the
same fixture; vtmhip_isp_chain_host, the expectation of the GPU tests, against the composition of restatement and oracle, which rests on no entry of the library."""
import ctypes as C
import os

import numpy as np
import pytest

import intra_util as iu
import isp_util as isp
import oracle_lib as ol
from vtm_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    ol.build_oracle()
    return lib.load()


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "isp.npz"))
    blocks, lp, rp = [], 0, 0
    for w, h, bd in z["blocks"]:
        blocks.append(dict(w=int(w), h=int(h), bd=int(bd), top=z["lines"][lp:lp + 2 * w + 1], left=z["lines"][lp + 2 * w + 1:lp + 2 * w + 2 * h + 2],
                           reco=z["recos"][rp:rp + w * h].reshape(h, w)))
        lp += 2 * w + 2 * h + 2
        rp += w * h
    cases, pp, qp, np_ = [], 0, 0, 0
    for blk, mode, split, avail in z["cases"]:
        b = blocks[blk]
        g = isp.geometry(b["w"], b["h"], int(split))
        nr, w, h = g["numRegions"], b["w"], b["h"]
        nxt = []
        for _ in range(1, nr):
            nt, nl = w + g["regW"] + 1, h + g["regH"] + 1
            nxt.append((z["next_lines"][np_:np_ + nt], z["next_lines"][np_ + nt:np_ + nt + nl]))
            np_ += nt + nl
        cases.append(dict(b=b, mode=int(mode), split=int(split), avail=int(avail), g=g, pred=z["preds"][pp:pp + w * h].reshape(h, w),
                          params=z["params"][qp:qp + 8 * nr].reshape(nr, 8), next=nxt))
        pp += w * h
        qp += 8 * nr
    assert pp == z["preds"].size and qp == z["params"].size and np_ == z["next_lines"].size
    return dict(z=z, blocks=blocks, cases=cases)


def test_struct_sizes(L):
    assert [L.vtmhip_isp_struct_size(i) for i in range(4)] == [C.sizeof(lib.IspJob), C.sizeof(lib.IspResult), C.sizeof(lib.IspGeom), -1]
    assert C.sizeof(lib.IspJob) == 32 and C.sizeof(lib.IspResult) == 72 and isp.RESULT_DTYPE.itemsize == 72


def test_geometry_of_every_shape(L):
    """CU::canUseISP, getISPSplitDim, the prediction regions and the transform pair over every W x H of 4 .. 64 (and a few sides outside)"""
    seen = set()
    for w in (2, 4, 8, 12, 16, 32, 64, 128):
        for h in (2, 4, 8, 12, 16, 32, 64, 128):
            for split in (0, 1, 2, 3):
                g = lib.IspGeom()
                st = L.vtmhip_isp_geometry(w, h, split, C.byref(g))
                ok = isp.can_use(w, h) and split in (1, 2)
                assert (st == lib.OK) == ok, (w, h, split)
                if ok:
                    e = isp.geometry(w, h, split)
                    assert {k: getattr(g, k) for k in e} == e, (w, h, split)
                    assert g.numParts == (2 if (w, h) in ((4, 8), (8, 4)) else 4) and g.partW * g.partH * g.numParts == w * h and g.partW * g.partH >= 16
                    th, tv = C.c_int(), C.c_int()
                    assert L.vtmhip_isp_tr_types(g.partW, g.partH, C.byref(th), C.byref(tv)) == lib.OK and (th.value, tv.value) == (g.typeHor, g.typeVer)
                    seen.add((g.partW, g.partH))
    assert {(1, 16), (2, 8), (16, 1), (8, 2), (1, 64), (64, 1), (2, 64), (64, 2), (64, 16), (16, 64)} <= seen
    assert len({(w, h) for w in isp.SIDES for h in isp.SIDES if isp.can_use(w, h)}) == 24


def test_params_against_the_reference(L, golden):
    """initPredIntraParams with ispMode set: the wide-angle shift from the CU, PDPC and angularScale from the region, no filter -- every region of every recorded case"""
    small_regions = 0
    for c in golden["cases"]:
        b, g = c["b"], c["g"]
        p = lib.IntraParams()
        assert L.vtmhip_isp_pred_params(b["w"], b["h"], g["regW"], g["regH"], c["mode"], C.byref(p)) == lib.OK
        got = [getattr(p, f) for f in iu.PARAM_FIELDS]
        e = isp.params(b["w"], b["h"], g["regW"], g["regH"], c["mode"])
        for r in range(g["numRegions"]):
            assert got == [int(v) for v in c["params"][r]], (b["w"], b["h"], c["mode"], c["split"], r, got, c["params"][r])
        assert got == [e[f] for f in iu.PARAM_FIELDS]
        assert p.refFilterFlag == 0 and p.interpolationFlag == 0
        small_regions += int(min(g["regW"], g["regH"]) < 4 and p.applyPDPC == 0)
    assert small_regions > 20            # regions of height 1 and 2 exist, and PDPC is off there
    p = lib.IntraParams()
    assert L.vtmhip_isp_pred_params(16, 16, 16, 8, 0, C.byref(p)) == lib.E_INVALID          # no split of 16x16 has such a region
    assert L.vtmhip_isp_pred_params(16, 16, 16, 4, 67, C.byref(p)) == lib.E_INVALID


def _region_lines(c, r):
    b, g = c["b"], c["g"]
    if r == 0:
        return b["top"][:b["w"] + g["regW"] + 1], b["left"][:b["h"] + g["regH"] + 1]
    return c["next"][r - 1]


def test_region_predictions_against_the_reference(L, golden):
    """predIntraAng on every region of every recorded case, from the lines the reference's own update left: the host entry and the restatement"""
    for c in golden["cases"]:
        b, g = c["b"], c["g"]
        for r in range(g["numRegions"]):
            x0, y0 = (0, r * g["regH"]) if c["split"] == isp.HOR else (r * g["regW"], 0)
            top, left = (np.ascontiguousarray(a, np.int16) for a in _region_lines(c, r))
            exp = c["pred"][y0:y0 + g["regH"], x0:x0 + g["regW"]]
            got = np.zeros((g["regH"], g["regW"]), np.int16)
            assert L.vtmhip_isp_pred_region_host(b["w"], b["h"], g["regW"], g["regH"], c["mode"], b["bd"], top.ctypes.data, left.ctypes.data, got.ctypes.data) == lib.OK
            assert np.array_equal(got, exp), (b["w"], b["h"], c["mode"], c["split"], c["avail"], r)
            assert np.array_equal(isp.predict_region(top, left, b["w"], b["h"], g["regW"], g["regH"], c["mode"], b["bd"]), exp), (b["w"], b["h"], c["mode"], c["split"], r)


def test_next_lines_against_the_reference(L, golden):
    """initIntraPatternChTypeISP, both splits and both availability branches: the host entry (reads over the CU's lines and the reconstruction) and the restatement
    (the reference's in-place update) against the lines the member left"""
    branches = set()
    for c in golden["cases"]:
        b, g = c["b"], c["g"]
        ref = isp.RefLines(b["top"], b["left"], b["w"], b["h"], c["split"], c["avail"])
        reco = np.ascontiguousarray(b["reco"], np.int16)
        top, left = np.ascontiguousarray(b["top"], np.int16), np.ascontiguousarray(b["left"], np.int16)
        for r in range(1, g["numRegions"]):
            x0, y0 = (0, r * g["regH"]) if c["split"] == isp.HOR else (r * g["regW"], 0)
            et, el = c["next"][r - 1]
            gt, gl = np.full(et.size + 2, iu.POISON, np.int16), np.full(el.size + 2, iu.POISON, np.int16)
            assert L.vtmhip_isp_next_lines_host(b["w"], b["h"], c["split"], r, c["avail"], top.ctypes.data, left.ctypes.data, reco.ctypes.data, gt.ctypes.data,
                                                gl.ctypes.data) == lib.OK
            assert np.array_equal(gt[:-2], et) and np.array_equal(gl[:-2], el), (b["w"], b["h"], c["split"], c["avail"], r)
            assert (gt[-2:] == iu.POISON).all() and (gl[-2:] == iu.POISON).all()
            ref.update(b["reco"].astype(np.int64), x0, y0, g["regW"], g["regH"])
            rt, rl = ref.lines(g["regW"], g["regH"])
            assert np.array_equal(rt, et) and np.array_equal(rl, el), (b["w"], b["h"], c["split"], c["avail"], r)
            branches.add((c["split"], c["avail"]))
    assert branches == {(1, 0), (1, 1), (2, 0), (2, 1)}
    z = np.zeros(200, np.int16)
    assert L.vtmhip_isp_next_lines_host(8, 8, 1, 0, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data) == lib.E_INVALID      # region 0 has the CU's lines
    assert L.vtmhip_isp_next_lines_host(8, 8, 2, 2, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data) == lib.E_INVALID      # 8x8 vertical: two regions


def test_oracle_at_the_narrow_shapes_against_the_reference(golden):
    """vo_fwd_2d / vo_quant / vo_dequant / vo_inv_2d at 1xN, 2xN, Nx1, Nx2, with DST7 on both sides, and with the mixed DCT2 / DST7 pairs of ISP"""
    O, z = ol.oracle(), golden["z"]
    pos = 0
    for w, h, bd, mts, qp, irap, s_ref in z["tr"]:
        w, h, bd, n = int(w), int(h), int(bd), int(w * h)
        t = isp.DST7 if mts == 2 else isp.DCT2
        per, rem = isp.qp_of(int(qp), bd)
        resi = np.ascontiguousarray(z["tr_resi"][pos:pos + n].reshape(h, w))
        coef, q, dq, s, rec = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_int32(), np.zeros((h, w), np.int16)
        assert O.vo_fwd_2d(ol.P(resi), w, w, h, bd, t, t, ol.P(coef)) == 0
        O.vo_quant(ol.P(coef), w, h, bd, per, rem, int(irap), 0, ol.P(q), None, C.byref(s))
        O.vo_dequant(ol.P(q), w, h, bd, per, rem, 0, ol.P(dq))
        assert O.vo_inv_2d(ol.P(dq), w, h, bd, t, t, ol.P(rec), w) == 0
        assert np.array_equal(coef, z["tr_coef"][pos:pos + n]) and np.array_equal(q, z["tr_q"][pos:pos + n]) and s.value == s_ref, (w, h, bd, mts)
        assert np.array_equal(dq, z["tr_dq"][pos:pos + n]) and np.array_equal(rec.reshape(-1), z["tr_rec"][pos:pos + n]), (w, h, bd, mts)
        pos += n
    pos = 0
    for w, h, bd, th, tv in z["mx"]:
        w, h, bd, n = int(w), int(h), int(bd), int(w * h)
        assert (int(th), int(tv)) == (isp.DST7 if 4 <= w <= 16 else isp.DCT2, isp.DST7 if 4 <= h <= 16 else isp.DCT2)
        resi = np.ascontiguousarray(z["mx_resi"][pos:pos + n].reshape(h, w))
        coef, rec = np.zeros(n, np.int32), np.zeros((h, w), np.int16)
        assert O.vo_fwd_2d(ol.P(resi), w, w, h, bd, int(th), int(tv), ol.P(coef)) == 0
        assert O.vo_inv_2d(ol.P(np.ascontiguousarray(z["mx_in"][pos:pos + n])), w, h, bd, int(th), int(tv), ol.P(rec), w) == 0
        assert np.array_equal(coef, z["mx_coef"][pos:pos + n]) and np.array_equal(rec.reshape(-1), z["mx_rec"][pos:pos + n]), (w, h, bd)
        pos += n


MODES = [0, 1, 2, 18, 34, 50, 66, 7, 61, 45, 23, 56]


def test_chain_host_against_the_composition(L):
    """every candidate of every shape up to 16x16, and a few of the larger ones, from the restatement and the oracle alone: prediction, levels, reconstruction and the
    three sums per sub-partition; the buffers in full against a second run; NULL predBase / levelsBase; a prefix of the table"""
    rng = np.random.default_rng(3)
    small = [(w, h) for w, h in isp.SHAPES if w <= 16 and h <= 16]
    shapes = [(w, h, (8, 10, 12)[i % 3]) for i, (w, h) in enumerate(small + [(32, 32), (64, 64), (4, 64), (64, 8), (8, 32), (32, 16)])]

    def jobs_of(i, b):
        n = 8 if b["w"] <= 16 and b["h"] <= 16 else 2
        return [(MODES[(5 * i + k) % len(MODES)], 1 + (k & 1), (k >> 1) & 1, (12, 27, 37, 51)[(i + (k >> 1)) % 4], (i + k) & 1) for k in range(n)]
    b = isp.make_batch(rng, shapes, jobs_of, org=lambda rng, blk: isp.smooth_org(rng, blk, 40) if blk["w"] == 16 else rng.integers(0, 1 << blk["bd"], (blk["h"], blk["w"])))
    st, got = b.run_host()
    assert st == lib.OK
    for k in range(b.n):
        b.check_composed(got, k)
    res = got["results"]
    assert any(int(r["absSum"][p]) == 0 for r in res for p in range(int(r["numParts"]))) and any(int(r["absSum"][0]) > 0 for r in res)
    st, bare = b.run_host(pred=False, levels=False)
    assert st == lib.OK
    isp.Batch.same(bare, got, pred=False, levels=False)
    st, part = b.run_host(n=b.n - 5)
    assert st == lib.OK and np.array_equal(part["results"][:b.n - 5], res[:b.n - 5]) and (part["results"][b.n - 5:].view(np.uint8) == isp.FILL).all()
    st, none = b.run_host(n=0)
    assert st == lib.OK and isp.Batch.untouched(none)
    lanes = C.c_int()
    assert L.vtmhip_isp_chain_lanes_host(C.addressof(b.blk_arr), len(b.blocks), C.addressof(b.job_arr), b.n, C.byref(lanes)) == lib.OK and lanes.value == 256


def test_chain_dependency_shows_in_the_expectation(L):
    """the later sub-partitions are predicted from the reconstruction: with the original in its place the composition gives another prediction"""
    rng = np.random.default_rng(4)
    b = isp.make_batch(rng, [(16, 16, 10), (8, 8, 8), (4, 16, 12)], lambda i, blk: [(m, s, 1, 37, 0) for m in (0, 1, 34, 50) for s in (1, 2)])
    got = b.host()
    differs = 0
    for k in range(b.n):
        blk, j = b.blocks[b.jobs[k][0]], b.job_arr[k]
        pred = got["pred"][j.predOff:j.predOff + blk["w"] * blk["h"]].reshape(blk["h"], blk["w"])
        differs += int(not np.array_equal(pred, b.composed(k, from_org=True)["pred"]))
    assert 2 * differs >= b.n


@pytest.mark.parametrize("name,defect", isp.DEFECTS, ids=[d[0] for d in isp.DEFECTS])
def test_chain_host_rejects_malformed_tables(L, name, defect):
    b = isp.base_batch()
    st, good = b.run_host()
    assert st == lib.OK and not isp.Batch.untouched(good)
    defect(b)
    st, got = b.run_host()
    assert st == lib.E_INVALID and isp.Batch.untouched(got)
    lanes = C.c_int(-7)
    assert L.vtmhip_isp_chain_lanes_host(C.addressof(b.blk_arr), len(b.blocks), C.addressof(b.job_arr), b.n, C.byref(lanes)) == lib.E_INVALID and lanes.value == -7
