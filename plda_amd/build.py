"""plda_amd/build.py -- builds plda_amd/lib/libplda_hip.so for gfx950 with hipcc.

hipcc cross-compiles without a GPU; the .so is kept in-tree (git-ignored) so it
travels to the GPU box with the snapshot.

`--diag` (build(diag=True)) builds the DIAGNOSTIC library plda_amd/lib/libplda_hip_diag.so from the same sources with
-DPLDA_DIAG=1 (objects under lib/diag/): it additionally contains the measurement arms of the trials GEMM (bounding arms
that return garbage scores, timeline and clock-stamp arms; csrc/common.hpp).  The profiling scripts and bench.py's
shader-clock reading load it (plda_amd._native.load(diag=True) / PLDA_LIB_DIAG=1); nothing else does.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
SO = os.path.join(LIBDIR, "libplda_hip.so")
SO_DIAG = os.path.join(LIBDIR, "libplda_hip_diag.so")
SOURCES = ["api.hip", "score.hip", "linalg.hip", "fit.hip", "frontend.hip", "eer.hip", "operand_slabs.hip", "lda.hip", "comm.hip", "eig_dc.hip", "hostio.hip", "transform.hip", "snorm.hip", "calib.hip", "dcf.hip", "rocch.hip", "topn.hip", "fusion.hip", "adapt.hip", "ahc.hip", "dense_pca.hip", "vbx.hip", "der.hip", "der_time.hip", "embed.hip", "spectral.hip", "partition.hip", "cosine.hip"]
HEADERS = [os.path.join(CSRC, "common.hpp"), os.path.join(CSRC, "layout.hpp"), os.path.join(CSRC, "trial_source.hpp"), os.path.join(CSRC, "hostio.hpp"), os.path.join(CSRC, "slab_walk.hpp"), os.path.join(CSRC, "sweep_mfma.inc"), os.path.join(CSRC, "score_bt4.inc"), os.path.join(CSRC, "score_bf16x3.inc"), os.path.join(CSRC, "syrk_blk.inc"), os.path.join(HERE, "..", "include", "plda_hip.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
         "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


# score.hip: the one-lane queue atomic of trials_gemm_bt4_kernel must stay ONE asynchronous instruction -- the atomic optimizer
# rewrites it into a wave reduction that reads the result back on the spot (a memory round trip in the MFMA stream); the
# tile fetch's two values are deliberately defined on one path only (score_bt4.inc: the warning is silenced by a pragma around
# that include, not for the file)
# fusion.hip: machine LICM hoists the fp64 constants of exp / log1p out of the element loop into registers that live through
# the whole walk.  With the pass ON (the compiler's default) the labelled pass reports, K = 1 .. 8: 126 / 156 / 164 / 190 /
# 197 / 223 / 249 / 256 VGPRs, scalar-register spills from K = 5 on (2 / 4 / 6 / 14) and at K = 8 19 spilled VGPRs = 80 bytes
# of scratch per lane; with it OFF 94 .. 244, no spill and no scratch anywhere (the table in csrc/fusion.hip).  It is a hidden
# LLVM option and applies to the whole file (the list, map and reduce kernels lose nothing they had: their loops hold no
# hoistable constants beyond the same exp / log1p ones; the instantiations with sides, K25, walk with the same account and
# report the same figures); if a toolchain drops it the build fails loudly on the unknown option --
# then remove it and accept the K >= 5 spills, or split the constants' live ranges by hand.  Reproduce the table with
#   hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -mllvm -disable-machine-licm \
#         -Rpass-analysis=kernel-resource-usage -c plda_amd/csrc/fusion.hip -o /dev/null
# Its effect on speed has not been measured apart from the rest (scripts/fusion_bench.py times the kernels as built).
# ahc.hip: the clustering is specified to the bit (tests/ahc_model.py): one fp64 addition and one fp64 division where the
# contract names them, so nothing may be contracted into a fused multiply-add
# spectral.hip: the graph, the selection of the pruning value and the k-means are specified to the operation
# (tests/spectral_model.py): a squared distance is a product and a sum, never a fused multiply-add
# embed.hip: a row's bits may not depend on the block shape or the input dtype's instantiation it runs in (the determinism rule
# of the embedding chain): every fused multiply-add there is written as fma(), nothing else may be contracted
# frontend.hip: variance pooling subtracts the utterance's first normalised frame y0 = x0 * inv from every y = x * inv; a fused
# x * inv - y0 would subtract the rounded product from the unrounded one, and a one-frame utterance's variance would not be 0
# (the fused multiply-adds the kernels do want are written as fma())
# cosine.hip: a row's packed bits are a function of the row and its own zstd alone, whichever launch shape runs, and they are
# specified to the operation (tests/cosine_model.py): a square is a product and a sum, nothing may be contracted
EXTRA = {"score.hip": ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None"],
         "frontend.hip": ["-ffp-contract=off"],
         "fusion.hip": ["-mllvm", "-disable-machine-licm"],
         "ahc.hip": ["-ffp-contract=off"],
         "embed.hip": ["-ffp-contract=off"],
         "spectral.hip": ["-ffp-contract=off"],
         "cosine.hip": ["-ffp-contract=off"]}


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, diag=False):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(LIBDIR, "diag") if diag else LIBDIR
    so = SO_DIAG if diag else SO
    flags = FLAGS + (["-DPLDA_DIAG=1"] if diag else [])
    os.makedirs(objdir, exist_ok=True)
    objs = []
    procs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + HEADERS):
            cmd = [hipcc] + flags + EXTRA.get(src, []) + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    failed = False
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            failed = True
            sys.stderr.write("hipcc failed on %s:\n%s\n" % (src, out))
        elif verbose and out.strip():
            print(out)
    if failed:
        raise RuntimeError("hipcc compilation failed")
    if force or procs or _stale(so, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so] + objs + ["-ldl", "-lpthread"]   # librccl is opened lazily by plda_comm_init (csrc/comm.hip)
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return so


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, diag="--diag" in sys.argv))
