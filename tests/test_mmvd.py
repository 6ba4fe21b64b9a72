"""CPU: the MMVD merge candidates on the host -- vtmhip_mmvd_cands_host (the rules of vtm_amd/csrc/mmvd_rules.hpp) and the plain-Python restatement of mmvd_util
against every case of tests/golden/mmvd.npz (recorded from the reference's own MergeCtx::setMmvdMergeCandiInfo by tests/golden/gen_mmvd_golden.py), the table predicate,
the struct sizes, and the candidate loop's rule."""
import ctypes as C
import os

import numpy as np
import pytest

import mmvd_util as mu
from vtm_amd import lib
from vtm_amd.lib import PicParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIC = (416, 240, 128)


@pytest.fixture(scope="module")
def L():
    return lib.load()


def golden_cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mmvd.npz"))
    for row, mv, small in zip(z["cases"], z["mv"], z["small"]):
        row = [int(v) for v in row]
        w, h, dis_frac = row[:3]
        bases = []
        for b in range(2):
            s = row[3 + 12 * b:15 + 12 * b]
            bases.append(mu.make_base(mv=((s[0], s[1]), (s[2], s[3])), ref_idx=(s[4], s[5]), poc_diff=(s[6], s[7]), long_term=(s[8], s[9]), alt_hpel=s[10], bcw=s[11],
                                      ref_stride=(w, w)))
        yield mu.make_job(w, h, bases, pos=(64, 64), dis_frac=dis_frac), mv, small


def test_golden_file_covers_the_issue_cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mmvd.npz"))
    c = z["cases"]
    assert len(c) == 3 * 7 * 3 * 2 * 3 * 4 * 2 and z["mv"].shape == (len(c), 64, 4) and z["small"].shape == (len(c), 64, 6)
    assert {(int(a), int(b)) for a, b in c[:, :2]} == {(8, 4), (4, 8), (8, 8), (16, 16)}
    assert set(c[:, 2]) == {0, 1} and set(c[:, 14]) == {4, 10}
    assert np.abs(z["mv"]).max() == 1 << 17                                    # the storage clip engages
    assert {(int(a) >= 0, int(b) >= 0) for a, b in c[:, 7:9]} == {(True, False), (False, True), (True, True)}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mmvd.npz")) < 200 * 1024


def test_restatement_and_host_entry_against_the_reference(L):
    pic = PicParams(PIC[0], PIC[1], PIC[2], 10)
    n = 0
    for job, mv, small in golden_cases():
        exp = mu.derive_all(job, PIC)
        st, got, pmv = mu.host_cands(L, job, pic)
        assert st == lib.OK
        for c in range(64):
            ref = tuple(int(v) for v in mv[c]) + tuple(int(v) for v in small[c][:5])
            assert mu.record_tuple(exp[c])[:9] == ref, (job, c)
            step = (c % 32) // 4
            bdof = bool(small[c][5]) and ref[6] == 3 and job["w"] >= 8 and job["h"] >= 8 and job["w"] * job["h"] >= 128 and ref[7] == 4 and step <= 2
            assert exp[c]["kind"] == (mu.BDOF if bdof else mu.PLAIN), (job, c)
            assert got[c] == mu.record_tuple(exp[c]), (job, c)
            assert pmv[c] == exp[c]["pred_mv"], (job, c)
        n += 1
    assert n == 3024


def test_the_golden_cases_reach_every_branch():
    """what the recorded cases must contain for the comparison above to mean something"""
    seen = dict(scaled_l0=0, scaled_l1=0, mirror=0, copy=0, equal=0, restricted=0, bdof=0, clip=0, identical=0)
    for job, mv, small in golden_cases():
        for k, b in enumerate(job["bases"]):
            if min(b["ref_idx"]) < 0:
                continue
            d0, d1 = b["poc_diff"]
            lt = max(b["long_term"])
            seen["equal"] += d0 == d1
            seen["mirror"] += bool(lt) and d0 != d1 and d0 * d1 < 0
            seen["copy"] += bool(lt) and d0 != d1 and d0 * d1 > 0
            seen["scaled_l0"] += (not lt) and abs(d1) > abs(d0)
            seen["scaled_l1"] += (not lt) and abs(d1) < abs(d0)
        seen["restricted"] += job["w"] + job["h"] == 12 and min(job["bases"][0]["ref_idx"]) >= 0
        seen["bdof"] += int(small[:, 5].any())
        seen["clip"] += int(np.abs(mv).max() == 1 << 17)
        seen["identical"] += any(c["inter_dir"] == 3 and c["pred_mode"] == mu.PRED_L0 for c in mu.derive_all(job, PIC))
    assert all(v > 0 for v in seen.values()), seen


def test_dist_scale_factor_and_scale_mv_edges():
    assert mu.dist_scale_factor(0, -2, 0, -2) == 4096
    assert mu.dist_scale_factor(0, 1, 0, -3) == (1 * mu.c_div(0x4000 + 1, 3) * -1 + 32 >> 6)      # tdb = -1, tdd = 3: C division of the odd half
    assert mu.dist_scale_factor(0, 150, 0, -200) == ((-128) * mu.c_div(0x4000 + 63, 127) + 32 >> 6)   # both differences clipped to -128 / 127
    assert mu.scale_mv([4, -4], -2048) == [(-8192 + 128) >> 8, (8192 + 127) >> 8]
    assert mu.c_div(-7, 2) == -3 and mu.c_div(7, -2) == -3


def test_prediction_vectors_are_clipped_at_the_picture_corner(L):
    pic = PicParams(PIC[0], PIC[1], PIC[2], 10)
    base = mu.make_base(mv=((40, 24), (0, 0)), ref_idx=(0, -1), ref_stride=(16, 16))
    job = mu.make_job(16, 16, [base], pos=(PIC[0] - 16, PIC[1] - 16), dis_frac=1)
    exp = mu.derive_all(job, PIC)
    st, got, pmv = mu.host_cands(L, job, pic)
    assert st == lib.OK and pmv == [c["pred_mv"] for c in exp]
    assert sum(c["pred_mv"][0] != c["mv"][0] for c in exp) >= 4
    assert all(c["pred_mv"][0][0] <= (8 + 16 - 1) * 16 and c["pred_mv"][0][1] <= (8 + 16 - 1) * 16 for c in exp)


@pytest.mark.parametrize("num_base,num_steps", [(1, 1), (1, 3), (1, 7), (2, 3), (2, 8), (1, 8)])
def test_loop_rule_leaves_the_reference_set_of_indices(L, num_base, num_steps):
    # the loop of EncCu.cpp:2528-2534, written out
    temp_num, ref_set = (64 if num_base > 1 else 32), set()
    for cand in range(temp_num):
        base_idx = cand // 32
        if (cand - base_idx * 32) // 4 >= num_steps:
            continue
        ref_set.add(cand)
    job = mu.make_job(16, 8, [mu.make_base(ref_idx=(0, 1), ref_stride=(16, 16))], num_base=num_base, num_steps=num_steps)
    st, got, pmv = mu.host_cands(L, job, PicParams(PIC[0], PIC[1], PIC[2], 10))
    assert st == lib.OK
    assert {c for c in range(64) if got[c][9] != mu.NOT_TESTED} == ref_set
    assert {c for c in range(64) if mu.derive(job, PIC, c)["kind"] != mu.NOT_TESTED} == ref_set
    for c in set(range(64)) - ref_set:
        assert got[c] == (0, 0, 0, 0, -1, -1, 0, 0, 0, 0) and pmv[c] == [[0, 0], [0, 0]]


def _good_job():
    return mu.make_job(16, 8, [mu.make_base(ref_idx=(0, 0), ref_stride=(16, 16)), mu.make_base(ref_idx=(-1, 1), ref_stride=(0, 16))])


MALFORMED = {
    "width 2": lambda j: j.update(w=2),
    "width 12": lambda j: j.update(w=12, org_stride=16),
    "width 256": lambda j: j.update(w=256, org_stride=256),
    "height 0": lambda j: j.update(h=0),
    "height 24": lambda j: j.update(h=24),
    "4 x 4": lambda j: j.update(w=4, h=4),
    "numBase 0": lambda j: j.update(num_base=0),
    "numBase 3": lambda j: j.update(num_base=3),
    "numSteps 0": lambda j: j.update(num_steps=0),
    "numSteps 9": lambda j: j.update(num_steps=9),
    "bitDepth 7": lambda j: j.update(bd=7),
    "bitDepth 13": lambda j: j.update(bd=13),
    "orgStride": lambda j: j.update(org_stride=15),
    "base 0 without a list": lambda j: j["bases"][0].update(ref_idx=[-1, -1]),
    "base 1 without a list": lambda j: j["bases"][1].update(ref_idx=[-1, -1]),
    "refStride of list 0": lambda j: j["bases"][0].update(ref_stride=[15, 16]),
    "refStride of list 1": lambda j: j["bases"][1].update(ref_stride=[0, 8]),
    "BCW weight 0": lambda j: j["bases"][0].update(bcw=0),
    "BCW weight 6": lambda j: j["bases"][1].update(bcw=6),
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_predicate_rejects_each_malformed_field(L, what):
    job = _good_job()
    assert mu.host_cands(L, job, PicParams(PIC[0], PIC[1], PIC[2], job["bd"]))[0] == lib.OK
    MALFORMED[what](job)
    assert mu.host_cands(L, job, PicParams(PIC[0], PIC[1], PIC[2], job["bd"] if 8 <= job["bd"] <= 12 else 10))[0] == lib.E_INVALID


def test_predicate_ignores_the_unused_base_and_checks_pic(L):
    job = _good_job()
    job["num_base"] = 1
    job["bases"][1].update(ref_idx=[-1, -1], bcw=0)
    assert mu.host_cands(L, job, PicParams(PIC[0], PIC[1], PIC[2], 10))[0] == lib.OK
    assert mu.host_cands(L, job, PicParams(PIC[0], PIC[1], PIC[2], 8))[0] == lib.E_INVALID      # the job's depth is not the picture's
    assert mu.host_cands(L, job, PicParams(0, PIC[1], PIC[2], 10))[0] == lib.E_INVALID


def test_struct_sizes_and_abi_version(L):
    assert L.vtmhip_abi_version() == 6
    assert [L.vtmhip_mmvd_struct_size(i) for i in range(4)] == [C.sizeof(lib.MmvdJob), C.sizeof(lib.MmvdCand), C.sizeof(lib.MmvdBase), -1]
    assert (C.sizeof(lib.MmvdJob), C.sizeof(lib.MmvdCand), C.sizeof(lib.MmvdBase)) == (144, 24, 56)
    # the existing lists have not moved
    assert len(lib._STRUCTS) == 36 and L.vtmhip_struct_size(len(lib._STRUCTS)) == -1
    assert [L.vtmhip_struct_size(i) for i in range(len(lib._STRUCTS))] == [C.sizeof(s) for s in lib._STRUCTS]
    assert [L.vtmhip_isp_struct_size(i) for i in range(4)] == [C.sizeof(s) for s in lib._ISP_STRUCTS] + [-1]
