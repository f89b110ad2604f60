"""CPU: the labelled fusion pass of plda_amd/csrc/fusion.hip, its own kernel text compiled for the host and run wave-lockstep
(tests/fusion_emu/emu.cpp), against the host model tests/fusion_model.py.

What this pins without a GPU is the LOGIC of fusion_pass_strip_kernel, fusion_block_store and fusion_reduce_kernel: a workgroup
walking several rows in steps of U = 4 / 2 / 1 with a partial last step (the emulation deals the rows over at most 8 slices, so
37 rows are 5 per workgroup, 46 are 6, 21 are 3), the inlined (K <= 2) and the rolled (K > 2) account, columns beyond the last one,
per-system pitches and alignments, the wave-cooperative target sum with whole waves of targets and with waves that hold none,
and the fixed-order reductions.  Integers and extremes exactly, sums within the band of tests/test_gpu_fusion.py (the host's
exp / log1p are the model's own, so the sums in fact agree to a few ulps).  The GPU's arithmetic is test_gpu_fusion.py's."""
import os
import re
import subprocess

import numpy as np
import pytest

import fusion_model as fm
from conftest import ROOT
from test_gpu_fusion import _compare, _labels, _placement, _points, _systems, _theta

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLANG = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang++")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.fail("the host compiler of the ROCm toolchain (%s) is missing: build() needs the same toolchain" % CLANG)
    d = tmp_path_factory.mktemp("fusion_emu")
    src = open(os.path.join(ROOT, "plda_amd", "csrc", "fusion.hip")).read()
    body = src[src.index("typedef float f32x4f"):src.index("// ------------------------------------------------------------------------------------ host drivers")]
    # what only the device compiler understands: the kernel-argument address space, the occupancy attribute, and the empty asm
    # whose "+s" / "+v" operands exist to stop hoisting (no instruction)
    body, n1 = re.subn(r"typedef const FusionArgs __attribute__\(\(address_space\(4\)\)\) \*FusionArgsPtr;", "typedef const FusionArgs *FusionArgsPtr;", body)
    body, n2 = re.subn(r'asm volatile\("" :[^;]*;', "", body)
    body = body.replace("__attribute__((amdgpu_waves_per_eu(2)))", "")
    assert n1 == 1 and n2 == 1
    (d / "kernels.inc").write_text(body)
    exe = str(d / "emu")
    subprocess.run([CLANG, "-O1", "-std=c++17", "-pthread", "-Wno-unused-result", "-I", str(d), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "fusion_emu", "emu.cpp"), "-o", exe], check=True, timeout=300)
    return d, exe


@pytest.mark.parametrize("m,nt,k,mode,layout", [(37, 130, 1, "all", "blocks"), (46, 66, 1, "none", "random"), (37, 130, 2, "one", "sparse"),
                                                (21, 70, 4, "one", "blocks"), (21, 261, 3, "one", "random"), (90, 1, 8, "all", "random"),
                                                (11, 70, 8, "one", "blocks")])
def test_emulated_pass_matches_the_model(emu, m, nt, k, mode, layout):
    from plda_amd import fusion as FU
    d, exe = emu
    rng = np.random.default_rng(m * 7919 + nt * 31 + k)
    es, ts = _labels(rng, m, nt, layout)
    tgt = es[:, None] == ts[None, :]
    S = _systems(rng, m, nt, k, tgt)
    lds, offs = _placement(k, nt, mode)
    for name, (a, c) in _points(S, tgt, k, ("cancel",)):
        theta = _theta(S, a, c)
        with open(d / "in.bin", "wb") as f:
            for j in range(k):
                f.write(np.int64(lds[j]).tobytes() + np.int64(offs[j]).tobytes())
            f.write(np.asarray(a, np.float64).tobytes() + np.float64(c).tobytes() + np.float64(theta).tobytes())
            f.write(es.tobytes() + ts.tobytes())
            for j in range(k):
                flat = np.full(offs[j] + m * lds[j], -7.25e30, np.float32)            # the padding is a value no sum survives
                flat[offs[j]:].reshape(m, lds[j])[:, :nt] = S[j]
                f.write(flat.tobytes())
        subprocess.run([exe, str(k), str(m), str(nt), str(d / "in.bin"), str(d / "out.bin")], check=True, timeout=600, capture_output=True)
        raw = np.fromfile(d / "out.bin", FU.RECORD_DTYPE)
        _compare("emulated %dx%d K %d %s %s at %s" % (m, nt, k, mode, layout, name), FU._record(raw), fm.pass_matrices(S, es, ts, a, c, theta))
        r = raw[0]                                                                 # entries beyond K are zero
        assert np.all(r["sum"]["G"][:, k + 1:] == 0) and np.all(r["sum"]["H"][:, fm.n_h(k):] == 0) and np.all(r["smin"][k:] == 0)
        assert int(r["n_systems"]) == k and int(r["reserved"]) == 0
