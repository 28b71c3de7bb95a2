"""Sign-bit hiding as the device decides it (thevc_amd/csrc/hmx_sbh.h), compiled for the host with g++ and held against the
oracle's xQuant with sign hiding on: two million random and adversarial 4x4 / 8x8 / 16x16 blocks over every scan, 8/10/12 bit,
QP 0-51, intra and inter rounding, the lastCG case and first levels of +-1 with deltaU <= 0.  Needs no GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_sbh_decision_equals_the_oracle(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    exe = str(tmp_path / "sbh_core_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "thevc_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(HERE, "native", "sbh_core_host.cpp"), "-o", exe, "-L", os.path.join(ROOT, "oracle"),
                           "-lhmx_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    r = subprocess.run([exe, "2000000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    assert "identical to the oracle" in r.stdout
