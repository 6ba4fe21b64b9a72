"""The CIIP rules of vtm_amd/csrc/ciip_rules.hpp and the host entries' bodies of ciip_host.hpp (both HIP-free) as a stand-alone program under AddressSanitizer and
UBSan: every CIIP size, weight and depth with every array in a heap allocation of exactly its length, every line index seen by INTRA_LINE_CHECK, and the predicate's
edge jobs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_ciip")


def _build():
    csrc = os.path.join(ROOT, "vtm_amd", "csrc")
    srcs = [os.path.join(ROOT, "host", "test_ciip.cpp"), os.path.join(ROOT, "include", "vtmhip.h")] + [os.path.join(csrc, n) for n in
                                                                                                       ("ciip_rules.hpp", "ciip_host.hpp", "intra_rules.hpp", "had_tile_rule.hpp")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", EXE, srcs[0]])


def test_ciip_rules_under_sanitizers():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " 0 outside" in r.stdout and " 0 failures" in r.stdout and "ciip rules: 440 blocks" in r.stdout      # 22 CIIP sizes x 5 depths x 4 flag pairs
