"""GPU parity of the round bound (tz_search_bound_kernel: candidates of the diamond, star and two-point rounds that the block-sum lower bound rules out are not
evaluated): the job sets of test_gpu_tz_prune -- 100-row sets of 128x128 and 128x64 rows on an 832x480 scene, the smallest shapes that take the bounded instantiations --
through vtmhip_xMotionEstimation_batch_dev against the oracle's records, with the box sums attached (bound on), with nothing attached, and (a child process) with
VTMHIP_TZ_ROUND_BOUND=0.  The context's statistic (vtmhip_tz_round_stats) says what the bound did; its `violations` counter is the kernel's own check that no evaluated
candidate's SAD came out below its bound."""
import os
import subprocess
import sys
import time

import pytest

import me_util
import test_gpu_tz_prune as prune
from test_gpu_tz_bands import CFGV, band_jobs
from test_gpu_tz_prune import SETS, case, run_device

ROUND_OFF = os.environ.get("VTMHIP_TZ_ROUND_BOUND") == "0"      # (the child of test_round_bound_switched_off)
NEW = ("first_rounds", "first_listed", "first_skipped", "resume_rounds", "resume_listed", "resume_skipped")

_ROUND = {}


def checked_runs(ctx, key, scene, jobs, exp, exp_int, w, h, wpj, copies=1):
    """The rows with the sums attached and with nothing attached against the expected records: (round statistic, prune statistic) of the attached run.  With nothing
    attached the new counters are all 0; no run has a violation."""
    t0 = time.time()
    exp, exp_int = exp * copies, exp_int * copies
    ctx.tz_round_stats(reset=True)
    got, got_int, st = run_device(ctx, scene, jobs, w, h, wpj, True, copies)
    rs = ctx.tz_round_stats(reset=True)
    bad = [k for k in range(len(exp)) if got[k] != exp[k] or got_int[k] != exp_int[k]]
    assert not bad, ("sums attached", rs, bad[:10], [(got[k], exp[k], got_int[k], exp_int[k], jobs[k % len(jobs)]["searchRange"]) for k in bad[:3]])
    got0, got_int0, st0 = run_device(ctx, scene, jobs, w, h, wpj, False, copies)
    rs0 = ctx.tz_round_stats(reset=True)
    assert got0 == exp and got_int0 == exp_int, ("nothing attached", rs0)
    print("round bound case", key, rs, "prune", st, "seconds %.2f" % (time.time() - t0))
    assert rs["violations"] == 0 and rs0["violations"] == 0, (rs, rs0)
    assert all(rs0[k] == 0 for k in NEW), rs0
    if ROUND_OFF:
        assert all(rs[k] == 0 for k in NEW), rs
    return rs, st, st0


def round_case(ctx, kind, w, h, wpj, copies=1):
    """One job set of test_gpu_tz_prune: its case() first (the oracle's records, cached per session, and the relations between the six old counters of the attached and
    the unattached run), then the two runs with the new statistic read."""
    key = (kind, w, h, wpj, copies)
    if key not in _ROUND:
        old = case(ctx, kind, w, h, wpj, copies)
        scene, jobs, exp, exp_int = prune._CASES[("oracle", kind, w, h)]
        rs, st, st0 = checked_runs(ctx, key, scene, jobs, exp, exp_int, w, h, wpj, copies)
        assert st == old, (st, old)      # the raster kernel sees the same searches
        assert st0["listed"] == st["listed"] and st0["accepted"] == st["accepted"] and st0["points_total"] == st["points_total"], (st, st0)
        _ROUND[key] = rs
    return _ROUND[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,w,h,wpj,copies", SETS)
def test_bounded_rounds_match_oracle(ctx, kind, w, h, wpj, copies):
    round_case(ctx, kind, w, h, wpj, copies)


@pytest.mark.gpu
def test_round_bound_is_not_vacuous(ctx):
    """Over the job sets: candidates skipped in the first and in the resume launches, something still evaluated, and a round skipped whole -- the statistic has no counter of
    its own for that, but a round that is not skipped whole evaluates at least one candidate, so listed - skipped < rounds in some launch kind of some set proves one.
    easy / easy_off8 (the search holds the exact motion when the refinement starts: every candidate but the match itself has a bound above the rate-only best cost): more
    than half of the resume launches' candidates are skipped."""
    tot = dict.fromkeys(NEW, 0)
    whole = []
    for s in SETS:
        rs = round_case(ctx, *s)
        for k in NEW:
            tot[k] += rs[k]
        for kind in ("first", "resume"):
            if rs[kind + "_rounds"] and rs[kind + "_listed"] - rs[kind + "_skipped"] < rs[kind + "_rounds"]:
                whole.append((s, kind))
        if s[0] in ("easy", "easy_off8"):
            print("round bound", s, "resume listed", rs["resume_listed"], "skipped", rs["resume_skipped"])
    print("round bound totals", tot, "sets with a round skipped whole", whole)
    if ROUND_OFF:      # (the whole file under VTMHIP_TZ_ROUND_BOUND=0: no round is bounded)
        assert not any(tot.values()), tot
        return
    assert tot["first_skipped"] > 0 and tot["resume_skipped"] > 0, tot
    assert tot["first_listed"] > tot["first_skipped"] and tot["first_listed"] + tot["resume_listed"] > tot["first_skipped"] + tot["resume_skipped"], tot
    assert whole, tot
    for s in SETS:
        if s[0] in ("easy", "easy_off8"):
            rs = round_case(ctx, *s)
            assert 2 * rs["resume_skipped"] > rs["resume_listed"], (s, rs)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,w,h,wpj", [("hard12", 128, 128, 8), ("hard", 64, 64, 4), ("hard", 128, 128, 4)])
def test_launches_the_bound_does_not_apply_to(ctx, kind, w, h, wpj):
    """12-bit samples (the 16-bit sums are not valid), 64x64 at four waves (subShift 1) and 128x128 at four waves (not a bounded instantiation) with sums attached: no round is
    bounded, the records match"""
    rs = round_case(ctx, kind, w, h, wpj)
    assert all(rs[k] == 0 for k in NEW), rs


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(128, 128), (128, 64)])
def test_flat_content(ctx, w, h):
    """Current and reference picture of one constant value: every SAD and every bound is 0 and the costs differ by the MV rate alone, so exact ties between a candidate
    and the best cost are the rule.  What this pins: the records equal the oracle's although the bound skips on nothing but the rate (a candidate at or above the best is
    skipped, one below it is evaluated and accepted), no violation, and candidates are in fact skipped.  What it does NOT pin: evaluating a tied candidate instead of
    skipping it (`<=` for `<` in round_bound_mask) changes no record -- tz_round rejects the tie anyway -- and only lowers the skipped count, whose exact value would take a
    host replica of the whole search flow to derive; the count is printed, not asserted."""
    scene = me_util.Scene(832, 480, hard=False, t_cur=4)
    scene.cur[...] = 500
    scene.ref_buf[...] = 500
    scene, jobs = band_jobs(w, h, 100, scene)
    exp, exp_int = me_util.run_oracle_mest(scene, jobs, CFGV)
    rs, _, _ = checked_runs(ctx, ("flat", w, h), scene, jobs, exp, exp_int, w, h, 8)
    if not ROUND_OFF:
        assert rs["first_listed"] > 0 and rs["first_skipped"] > 0, rs


@pytest.mark.gpu
def test_round_bound_switched_off():
    """VTMHIP_TZ_ROUND_BOUND=0 (read once per process: a child process): the parity test of every job set with sums attached -- the new counters all 0 (checked_runs), the
    same records."""
    env = dict(os.environ, VTMHIP_TZ_ROUND_BOUND="0")      # (the child runs the parity tests alone: -k)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "match_oracle"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "%d passed" % len(SETS) in out, out[-3000:]
