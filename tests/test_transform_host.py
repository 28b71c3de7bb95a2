"""The transform passes the kernels share with the host (thevc_amd/csrc/hmx_transform.h) on the CPU: tests/native/transform_host.cpp
compiles the header with g++ and holds every pass, in every form, against the plain matrix product written out in the program (see
its head for the sizes, shifts and inputs).  Built twice: as it is, and with -fsanitize=undefined,address as a plain program with
its own main.  No GPU is needed."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_passes_against_the_matrix_product(tmp_path, flags):
    out = str(tmp_path / "transform_host")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "thevc_amd", "csrc"),
                           os.path.join(HERE, "native", "transform_host.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-1500:])
    # 5 form masks x 5 transforms x 3 bit depths x (2 forward passes per forward input + 3 passes per inverse input)
    assert int(r.stdout) > 5 * 5 * 3 * 5 * 3000
