"""The ISP rules of vtm_amd/csrc/isp_rules.hpp and the host chain of isp_host.hpp (HIP-free) as a stand-alone program under AddressSanitizer and UBSan: every table in a
heap array of exactly its length, every index of a prediction's line reads and of the line update's reads watched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_isp")


def _build():
    csrc = os.path.join(ROOT, "vtm_amd", "csrc")
    srcs = [os.path.join(ROOT, "host", "test_isp.cpp")] + [os.path.join(csrc, n) for n in ("isp_host.hpp", "isp_rules.hpp", "intra_rules.hpp", "chain_rules.hpp",
                                                                                           "chroma_taps.hpp", "tr_tables.hpp")] + [os.path.join(ROOT, "include", "vtmhip.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", EXE, srcs[0]])


def test_isp_rules_and_host_chain_under_sanitizers():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout and " 0 outside their line" in r.stdout and " reads of the line update" in r.stdout
