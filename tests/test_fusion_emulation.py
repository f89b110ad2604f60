"""CPU: the labelled fusion pass of plda_amd/csrc/fusion.hip, its own kernel text compiled for the host and run wave-lockstep
(tests/fusion_emu/emu.cpp), against the host model tests/fusion_model.py.

What this pins without a GPU is the LOGIC of fusion_pass_strip_kernel, fusion_block_store and fusion_reduce_kernel: a workgroup
walking several rows in steps of U = 4 / 2 / 1 with a partial last step (the emulation deals the rows over at most 8 slices, so
37 rows are 5 per workgroup, 46 are 6, 21 are 3), the inlined (K <= 2) and the rolled (K > 2) account, columns beyond the last one,
per-system pitches and alignments, the wave-cooperative target sum with whole waves of targets and with waves that hold none,
and the fixed-order reductions.  Integers and extremes exactly, sums within the band of tests/test_gpu_fusion.py (the host's
exp / log1p are the model's own, so the sums in fact agree to a few ulps).  The GPU's arithmetic is test_gpu_fusion.py's.

The SIDE BRANCH of the same walk (K25, SIDES = true) is held to the contract of tests/test_gpu_fusion_side.py without a GPU:
the emulated pass over K matrices and Q sides gives the 1024 bytes of the emulated pass over K + Q matrices in which the sides
are materialised (plda_amd.fusion.side_values), and that record passes the comparison with the model as well."""
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
    # what only the device compiler understands: the kernel-argument address space (of FusionArgsPtr, FusionSideArgsPtr and
    # SideEnrolPtr), the occupancy attribute, and the empty asm (one in the pass, one in the map) whose "+s" / "+v" operands
    # exist to stop hoisting (no instruction)
    body, n1 = re.subn(r"typedef const (\w+) __attribute__\(\(address_space\(4\)\)\) \*(\w+);", r"typedef const \1 *\2;", body)
    body, n2 = re.subn(r'asm volatile\("" :[^;]*;', "", body)
    body = body.replace("__attribute__((amdgpu_waves_per_eu(2)))", "")
    assert n1 == 3 and n2 == 2
    (d / "kernels.inc").write_text(body)
    exe = str(d / "emu")
    subprocess.run([CLANG, "-O1", "-std=c++17", "-pthread", "-Wno-unused-result", "-I", str(d), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "fusion_emu", "emu.cpp"), "-o", exe], check=True, timeout=300)
    return d, exe


def _write_matrices(f, m, nt, S, lds, offs):
    for j, s in enumerate(S):
        flat = np.full(offs[j] + m * lds[j], -7.25e30, np.float32)            # the padding is a value no sum survives
        flat[offs[j]:].reshape(m, lds[j])[:, :nt] = s
        f.write(flat.tobytes())


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
            _write_matrices(f, m, nt, S, lds, offs)
        subprocess.run([exe, str(k), str(m), str(nt), str(d / "in.bin"), str(d / "out.bin")], check=True, timeout=600, capture_output=True)
        raw = np.fromfile(d / "out.bin", FU.RECORD_DTYPE)
        _compare("emulated %dx%d K %d %s %s at %s" % (m, nt, k, mode, layout, name), FU._record(raw), fm.pass_matrices(S, es, ts, a, c, theta))
        r = raw[0]                                                                 # entries beyond K are zero
        assert np.all(r["sum"]["G"][:, k + 1:] == 0) and np.all(r["sum"]["H"][:, fm.n_h(k):] == 0) and np.all(r["smin"][k:] == 0)
        assert int(r["n_systems"]) == k and int(r["reserved"]) == 0


# The side branch, at the smallest shapes that enter each path of the walk with T = K + Q feature slots:
#   37 x 130, T = 2: the inlined account, U = 4 with a partial last step (5 rows per workgroup), the tail strip's lanes beyond column 130;
#   21 x 261, T = 3: the rolled account, U = 2; side 1's test vector one float off a 16-byte boundary, so that slot takes scalar
#       loads while side 0's takes 16-byte ones;
#   11 x 70,  T = 8: U = 1, every op;
#   90 x 1,   T = 8: every slot scalar, three of every thread's four lanes beyond the last column -- and the test vectors'
#       padding there is NaN, which an enrol value would carry into a sum through 0 * NaN were it not replaced by 0.f.
SIDE_CASES = [(37, 130, 1, ("min",), (0,), "none", "blocks", False),
              (21, 261, 1, ("absdiff", "prod"), (0, 1), "one", "random", False),
              (11, 70, 3, ("min", "max", "sum", "absdiff", "prod"), (0, 1, 0, 1, 0), "one", "blocks", False),
              (90, 1, 1, ("max", "sum", "min", "absdiff", "prod", "max", "sum"), (0, 1, 0, 0, 1, 0, 1), "all", "random", True)]


@pytest.mark.parametrize("m,nt,k,ops,toffs,mode,layout,nan_pad", SIDE_CASES)
def test_emulated_side_pass_is_the_emulated_matrix_pass(emu, m, nt, k, ops, toffs, mode, layout, nan_pad):
    from plda_amd import fusion as FU
    d, exe = emu
    q = len(ops)
    rng = np.random.default_rng(m * 7919 + nt * 31 + k * 9 + q)
    es, ts = _labels(rng, m, nt, layout)
    tgt = es[:, None] == ts[None, :]
    S = _systems(rng, m, nt, k, tgt)
    qe = [(np.log(rng.uniform(2, 40, m)) - 1.0).astype(np.float32) for _ in ops]       # log-durations and the like, some negative
    qt = [(np.log(rng.uniform(2, 40, nt)) - 1.0).astype(np.float32) for _ in ops]
    mats = [FU.side_values(op, e[:, None], t[None, :]) for op, e, t in zip(ops, qe, qt)]
    assert all(x.dtype == np.float32 and x.shape == (m, nt) for x in mats)
    feats = S + mats
    lds, offs = _placement(k + q, nt, mode)
    for name, (a, c) in _points(feats, tgt, k + q, ("cancel",)):
        theta = _theta(feats, a, c)
        tail = np.asarray(a, np.float64).tobytes() + np.float64(c).tobytes() + np.float64(theta).tobytes() + es.tobytes() + ts.tobytes()
        with open(d / "side.bin", "wb") as f:
            for j in range(k):
                f.write(np.int64(lds[j]).tobytes() + np.int64(offs[j]).tobytes())
            padded = []
            for op, t, off in zip(ops, qt, toffs):
                flat = np.full(off + (nt + 3) // 4 * 4 + 4, np.nan if nan_pad else -7.25e30, np.float32)
                flat[off:off + nt] = t
                padded.append(flat)
                f.write(np.int64(FU.SIDE_OPS.index(op)).tobytes() + np.int64(off).tobytes() + np.int64(flat.shape[0]).tobytes())
            f.write(tail)
            _write_matrices(f, m, nt, S, lds, offs)
            for e, flat in zip(qe, padded):
                f.write(e.tobytes() + flat.tobytes())
        with open(d / "mat.bin", "wb") as f:
            for j in range(k + q):
                f.write(np.int64(lds[j]).tobytes() + np.int64(offs[j]).tobytes())
            f.write(tail)
            _write_matrices(f, m, nt, feats, lds, offs)
        subprocess.run([exe, str(k), str(m), str(nt), str(d / "side.bin"), str(d / "side.out"), str(q)], check=True, timeout=600, capture_output=True)
        subprocess.run([exe, str(k + q), str(m), str(nt), str(d / "mat.bin"), str(d / "mat.out")], check=True, timeout=600, capture_output=True)
        side, mat = np.fromfile(d / "side.out", FU.RECORD_DTYPE), np.fromfile(d / "mat.out", FU.RECORD_DTYPE)
        assert side.nbytes == 1024
        assert side.tobytes() == mat.tobytes(), [n for n in FU.RECORD_DTYPE.names if side[n].tobytes() != mat[n].tobytes()]
        _compare("emulated %dx%d K %d Q %d %s at %s" % (m, nt, k, q, ops, name), FU._record(side), fm.pass_matrices(feats, es, ts, a, c, theta))
        assert int(side["n_systems"][0]) == k + q and int(side["nonfinite"][0]) == 0
