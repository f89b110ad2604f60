"""CPU: the scratch-layout helper plda_amd/csrc/layout.hpp, which gives every multi-array device buffer of the library its
size and its pointers from one list.  tests/layout_check/check.cpp is compiled with the ROCm toolchain's host compiler under the
address and undefined-behaviour sanitizers and run as a child process (the header includes nothing of HIP)."""
import os
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLANG = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang++")


def test_layout_helper_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.fail("the host compiler of the ROCm toolchain (%s) is missing: build() needs the same toolchain" % CLANG)
    exe = str(tmp_path / "layout_check")
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "plda_amd", "csrc"), os.path.join(ROOT, "tests", "layout_check", "check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "layout ok", r.stdout + r.stderr
