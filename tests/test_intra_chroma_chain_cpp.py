"""The table rules of vtm_amd/csrc/intra_chroma_chain_rules.hpp (HIP-free: the checks and the job expansion of the intra chroma residual chain) as a stand-alone
program under AddressSanitizer and UBSan, every table in a heap array of exactly its length."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_intra_chroma_chain")


def _build():
    csrc = os.path.join(ROOT, "vtm_amd", "csrc")
    srcs = [os.path.join(ROOT, "host", "test_intra_chroma_chain.cpp")] + [os.path.join(csrc, h) for h in ("intra_chroma_chain_rules.hpp", "chain_rules.hpp", "cclm_rules.hpp", "intra_rules.hpp")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", EXE, srcs[0]])


def test_intra_chroma_chain_rules_under_sanitizers():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "0 failures" in r.stdout and "49 of 49 malformed tables rejected" in r.stdout
