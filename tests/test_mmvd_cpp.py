"""The MMVD rules of vtm_amd/csrc/mmvd_rules.hpp (HIP-free) as a stand-alone program under AddressSanitizer and UBSan: the derivation over randomised jobs, every
table in a heap array of exactly its length, and the table predicate."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_mmvd")


def _build():
    srcs = [os.path.join(ROOT, "host", "test_mmvd.cpp"), os.path.join(ROOT, "vtm_amd", "csrc", "mmvd_rules.hpp"), os.path.join(ROOT, "include", "vtmhip.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", EXE, srcs[0]])


def test_mmvd_rules_under_sanitizers():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "20000 jobs" in r.stdout and " 0 failures" in r.stdout
