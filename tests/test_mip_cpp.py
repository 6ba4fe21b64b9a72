"""The MIP rules of vtm_amd/csrc/mip_rules.hpp (HIP-free: shape, reduced boundaries, the matrix product, the closed-form up-sampling) as a stand-alone program
under AddressSanitizer and UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_mip")


def _build():
    srcs = [os.path.join(ROOT, "host", "test_mip.cpp"), os.path.join(ROOT, "vtm_amd", "csrc", "mip_rules.hpp")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", EXE, srcs[0]])


def test_mip_rules_under_sanitizers():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "0 failures" in r.stdout and " 0 outside their line" in r.stdout
