"""The GEO rules of vtm_amd/csrc/geo_rules.hpp and the host entries' bodies of geo_host.hpp (both HIP-free) as a stand-alone program under AddressSanitizer and
UBSan, compiled without contraction as the device code is: every eligible shape, depth and candidate count with every array in a heap allocation of exactly its
length, the three list regimes, the tie order and the predicate's edge jobs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_geo_cand")


def _build():
    csrc = os.path.join(ROOT, "vtm_amd", "csrc")
    srcs = [os.path.join(ROOT, "host", "test_geo_cand.cpp"), os.path.join(ROOT, "include", "vtmhip.h")] + [os.path.join(csrc, n) for n in
                                                                                                           ("geo_rules.hpp", "geo_host.hpp", "ciip_host.hpp", "had_tile_rule.hpp")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", EXE, srcs[0]])


def test_geo_rules_under_sanitizers():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "geo rules: 350 jobs, 0 failures" in r.stdout and "geo predicate: 12 rejected, 3 accepted" in r.stdout      # 14 shapes x 5 depths x 5 candidate counts
