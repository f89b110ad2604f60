"""CPU: the slab walk of the clustering family's operand forms (plda_amd/csrc/slab_walk.hpp), compiled on its own with the ROCm
toolchain's host compiler (tests/slab_walk/walk.cpp) and compared with a restatement of the rule: a recording of N segments
takes round_up(N * N, 64) floats, consecutive recordings share a slab while they fit the budget (cur + f == budget still fits),
and a recording larger than the budget gets a slab of its own.  score_ahc, score_spectral and score_dense_pca_ahc all place
their blocks by it, and score_dense_pca_ahc hands boff[] with its closing entry to the AHC's matrix form as block_off.

The same program is built once more with -fsanitize=address,undefined and run on the same cases."""
import os
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLANG = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang++")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def walk_exe(request, tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.fail("the host compiler of the ROCm toolchain (%s) is missing: build() needs the same toolchain" % CLANG)
    exe = str(tmp_path_factory.mktemp("slab_walk") / "walk")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([CLANG, "-O1", "-std=c++17", "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "plda_amd", "csrc"),
                    os.path.join(ROOT, "tests", "slab_walk", "walk.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def _rule(budget, sizes):
    runs, r0 = [], 0
    while r0 < len(sizes):
        r1, cur, boff = r0, 0, []
        while r1 < len(sizes):
            f = (sizes[r1] * sizes[r1] + 63) // 64 * 64
            if cur and cur + f > budget:
                break
            boff.append(cur)
            cur += f
            r1 += 1
        runs.append([r0, r1] + boff + [cur])
        r0 = r1
    return runs


# padded sizes: n = 1, 3 -> 64; 8 -> 64; 9 -> 128; 16 -> 256
CASES = [(1000, [9]),                    # R = 1
         (10, [9]),                      # R = 1, larger than the budget
         (32, [3, 9, 8, 1]),             # a budget below every recording: each alone
         (320, [8, 16, 3]),              # 64 + 256 fills the budget exactly: [0, 2) stays one run
         (319, [8, 16, 3]),              # one float less: it breaks behind the first recording
         (384, [8, 16, 3]),              # everything in one run
         (448, [1, 3, 9, 8, 16, 16, 9, 1, 1, 3]),
         (1 << 29, [1, 3, 9, 8, 16])]    # the default budget's order of magnitude


@pytest.mark.parametrize("budget,sizes", CASES)
def test_walk_is_the_rule(walk_exe, budget, sizes):
    out = subprocess.run([walk_exe, str(budget)] + [str(n) for n in sizes], check=True, timeout=60, capture_output=True, text=True).stdout
    lines = [[int(x) for x in ln.split()] for ln in out.splitlines()]
    want = _rule(budget, sizes)
    assert lines[0] == [max(run[-1] for run in want), len(want)]
    assert lines[1:] == want + want                                  # the walk, and the rewound walk
    for run in want:
        assert len(run) - 2 == run[1] - run[0] + 1                   # one entry per block and the closing one
    assert want[0][0] == 0 and want[-1][1] == len(sizes) and all(a[1] == b[0] for a, b in zip(want, want[1:]))


def test_the_cases_are_the_ones_meant():
    assert [len(_rule(b, s)) for b, s in CASES] == [1, 1, 4, 2, 3, 1, 4, 1]
    assert all(run[1] - run[0] == 1 for run in _rule(32, [3, 9, 8, 1])) and max(run[-1] for run in _rule(32, [3, 9, 8, 1])) == 128
    assert _rule(320, [8, 16, 3])[0] == [0, 2, 0, 64, 320] and _rule(319, [8, 16, 3])[0] == [0, 1, 0, 64]
