"""CPU: host-side logic of the shim (argument checks mirror pldamodule.cpp's ValueErrors), the row
partition of the trials matrix (plda_shard_plan through the C ABI) and the host transport of the
library's collectives on a 2-process gloo group."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from plda_amd import libplda
from plda_amd.sharding import shard_rows


def test_feature_and_label_checks():
    x = np.random.default_rng(0).random((6, 3))
    assert libplda._features(x.astype(np.float32)).dtype == np.float64          # quirk Q12 superset
    assert libplda._features(np.asfortranarray(x)).flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError, match="not floats"):
        libplda._features((x * 9).astype(np.int32))                               # pldamodule.cpp:59-62
    with pytest.raises(TypeError):
        libplda._features([[1.0, 2.0]])                                           # "O!" parse
    with pytest.raises(ValueError, match="not an unsigned"):
        libplda._labels(np.arange(6), 6)                                          # :55-58 / :133-136
    with pytest.raises(ValueError, match="not strings"):
        libplda._labels(np.array(["a"] * 6), 6, allow_strings_msg=True)           # :128-131
    with pytest.raises(ValueError, match="number of samples"):
        libplda._labels(np.arange(5, dtype=np.uint8), 6)
    y = libplda._labels(np.arange(6, dtype=np.uint16), 6)
    assert y.dtype == np.uint64 and y.flags["C_CONTIGUOUS"]


@pytest.mark.parametrize("m,world", [(10, 1), (10, 3), (7, 8), (100000, 8), (40000, 8), (5, 5)])
def test_shard_rows_partition(m, world):
    spans = [shard_rows(m, world, r) for r in range(world)]
    assert spans[0][0] == 0 and spans[-1][1] == m
    for (a, b), (c, d) in zip(spans, spans[1:]):
        assert b == c and b >= a and d >= c
    sizes = [b - a for a, b in spans]
    assert max(sizes) - min(sizes) <= 1


# ---- the HOST transport of the library's collectives (plda_host_collectives over gloo), world size 2 on CPU.
#      On the GPU box the very same callbacks carry csrc/comm.hip's collectives between processes
#      (tests/test_gpu_comm_procs.py); here they are driven directly on host buffers. ----
def _transport_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import ctypes as C
    from plda_amd import _native as N
    from plda_amd.libplda import MPlda
    from plda_amd.sharding import TorchHostTransport
    tr = TorchHostTransport()
    t = tr.table
    ok = {}
    # ragged all-gather in place: rank q owns bytes [offs[q], offs[q] + counts[q]) of the same buffer
    for name, counts in [("ragged", [1000, 37]), ("empty_piece", [0, 513]), ("equal", [256, 256]), ("big", [3 << 20, (3 << 20) + 5])]:
        offs = [64, 64 + counts[0] + 11]                       # pieces need not be adjacent
        total = offs[1] + counts[1]
        want = np.zeros(total, np.uint8)
        for r in range(world):
            want[offs[r]:offs[r] + counts[r]] = (np.arange(counts[r]) * (r + 3) + r) % 251
        buf = np.zeros(total, np.uint8)
        buf[offs[rank]:offs[rank] + counts[rank]] = want[offs[rank]:offs[rank] + counts[rank]]
        o, c = (C.c_int64 * world)(*offs), (C.c_int64 * world)(*counts)
        rc = t.all_gather_v(None, buf.ctypes.data, o, c)
        ok["agv_" + name] = rc == 0 and np.array_equal(buf, want)
    # reductions: f64 sum, u64 sum (the EER histograms), u32 max / min (its bracket)
    a = np.arange(1000, dtype=np.float64) * (rank + 1)
    ok["sum_f64"] = t.all_reduce(None, a.ctypes.data, a.size, N.PLDA_DT_F64, N.PLDA_OP_SUM) == 0 and \
        np.array_equal(a, np.arange(1000, dtype=np.float64) * 3)
    u = (np.arange(4096, dtype=np.uint64) << np.uint64(40)) + np.uint64(rank)
    ok["sum_u64"] = t.all_reduce(None, u.ctypes.data, u.size, N.PLDA_DT_U64, N.PLDA_OP_SUM) == 0 and \
        np.array_equal(u, (np.arange(4096, dtype=np.uint64) << np.uint64(41)) + np.uint64(1))
    w = np.array([7 + 100 * rank, 4000000000 - rank], np.uint32)
    lo, hi = w.copy(), w.copy()
    ok["max_u32"] = t.all_reduce(None, hi.ctypes.data, 2, N.PLDA_DT_U32, N.PLDA_OP_MAX) == 0 and hi.tolist() == [107, 4000000000]
    ok["min_u32"] = t.all_reduce(None, lo.ctypes.data, 2, N.PLDA_DT_U32, N.PLDA_OP_MIN) == 0 and lo.tolist() == [7, 3999999999]
    # a failing callback reports 1 and keeps the exception; nothing propagates into the C caller
    ok["bad_dtype"] = t.all_reduce(None, a.ctypes.data, 4, 99, N.PLDA_OP_SUM) == 1 and isinstance(tr.last_error, ValueError)
    # the partition each rank computes for itself (plda_shard_plan through the C ABI) tiles the rows
    plans = [None] * world
    dist.all_gather_object(plans, MPlda.shard_plan(2900, world, rank, 256))
    cover = np.zeros(2900, np.int32)
    for pl in plans:
        for x, y in pl:
            cover[x:y] += 1
    ok["plans_tile"] = bool((cover == 1).all())
    q.put((rank, ok))
    dist.barrier()
    dist.destroy_process_group()


def test_host_transport_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_transport_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in procs), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok in res:
        assert all(ok.values()), (rank, ok)


def test_shard_plan_capacity_and_arguments():
    """plda_shard_plan is a pure function of the library (no handle, no GPU)."""
    import ctypes as C
    from plda_amd import _native as N
    lib = N.load()
    nb, rows = C.c_int64(), C.c_int64()
    assert lib.plda_shard_plan(100000, 8, 3, 4096, None, None, 0, C.byref(nb), C.byref(rows)) == N.PLDA_OK
    assert nb.value == 4 and rows.value == 3 * 4096 + 256          # 3 full rounds + a 1696-row tail in blocks of 256
    st, ct = np.zeros(2, np.int64), np.zeros(2, np.int64)
    assert lib.plda_shard_plan(100000, 8, 3, 4096, st.ctypes.data, ct.ctypes.data, 2, C.byref(nb), C.byref(rows)) == N.PLDA_E_CAPACITY
    assert st.tolist() == [3 * 4096, 8 * 4096 + 3 * 4096] and ct.tolist() == [4096, 4096]
    assert lib.plda_shard_plan(10, 0, 0, 256, None, None, 0, None, None) == N.PLDA_E_INVAL
    assert lib.plda_shard_plan(10, 2, 2, 256, None, None, 0, None, None) == N.PLDA_E_INVAL
    assert lib.plda_shard_plan(0, 2, 1, 256, None, None, 0, C.byref(nb), C.byref(rows)) == N.PLDA_OK and nb.value == 0


def test_block_cyclic_rows_tile_exactly():
    """plda_score_matrix_sharded_dev's partition (csrc/comm.hip, read through plda_shard_plan): every row belongs to
    exactly one rank, blocks are multiples of 256 rows, the remainder is dealt out in equal smaller blocks."""
    from plda_amd.sharding import block_cyclic_rows
    for m, world, block in [(1, 1, 256), (5, 4, 256), (2900, 2, 256), (2900, 3, 512), (2900, 8, 256),
                            (100000, 8, 4096), (100000, 2, 4096), (40000, 8, 4096), (40000, 4, 0), (4096 * 8, 8, 4096)]:
        cover = np.zeros(m, np.int32)
        sizes = []
        for r in range(world):
            rows = block_cyclic_rows(m, world, r, block)
            for a, b in rows:
                assert 0 <= a < b <= m and a % 256 == 0
                cover[a:b] += 1
            sizes.append(sum(b - a for a, b in rows))
        assert (cover == 1).all(), (m, world, block)
        blk = -(-(block if block > 0 else 4096) // 256) * 256
        assert max(sizes) - min(sizes) <= max(blk, 256), (m, world, block, sizes)   # balanced to within one block


def test_label_compaction_matches_unique():
    """fit()'s host-side label compaction (counting for small integer labels, already-dense labels untouched, np.unique
    for wide ones) gives what np.unique(return_inverse=True) gives: dense ids in ascending label order."""
    from plda_amd.libplda import _compact_labels
    rng = np.random.default_rng(5)
    cases = [np.repeat(np.arange(50, dtype=np.uint64), 7),                              # dense, sorted
             rng.permutation(np.repeat(np.arange(50, dtype=np.uint64), 7)),             # dense, shuffled
             rng.choice(np.array([3, 17, 18, 400, 2000], np.uint64), 300),              # sparse small integers
             rng.integers(0, 2 ** 63, 200, dtype=np.uint64) * np.uint64(2) + np.uint64(1),   # beyond int64: sort path
             np.full(10, 7, np.uint64),                                                  # one speaker
             np.array([2 ** 64 - 1, 0, 2 ** 64 - 1], np.uint64)]
    for y in cases:
        dense, k = _compact_labels(np.ascontiguousarray(y))
        uniq, inv = np.unique(y, return_inverse=True)
        assert k == uniq.shape[0]
        assert dense.dtype == np.uint64 and np.array_equal(dense, inv.astype(np.uint64))


def test_bench_launches_its_own_ranks(monkeypatch):
    """`python bench.py --gpus N` (N > 1) with no launcher around it must become the launcher -- the form the driver uses
    (torch.distributed.run, one process per GPU, rendezvous on 127.0.0.1) -- and never run ONE rank that prints
    n_gpus: 1 (round-4 review).  Without enough GPUs for the RCCL transport it refuses with a non-zero status."""
    import importlib
    import subprocess
    bench = importlib.import_module("bench")
    cmd = bench.launch_command(8, ["--gpus", "8", "--steps", "3"], port=29999)
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29999" and cmd[-4:] == ["--gpus", "8", "--steps", "3"]
    assert os.path.basename(cmd[-5]) == "bench.py"
    p1 = bench.launch_command(2, [])
    assert 1024 < int(p1[p1.index("--master-port") + 1]) < 65536         # a free port is picked when none is given
    # the launcher is what runs, not main()'s single-rank body
    calls = []
    monkeypatch.setattr(subprocess, "call", lambda c, env=None: calls.append((c, env)) or 0)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bench.self_launch(2, ["--gpus", "2", "--backend", "gloo", "--transport", "host"], transport="host") == 0
    assert len(calls) == 1 and calls[0][0][-6:] == ["--gpus", "2", "--backend", "gloo", "--transport", "host"]
    assert calls[0][1]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    import torch
    if torch.cuda.device_count() < 2:
        calls.clear()
        assert bench.self_launch(2, ["--gpus", "2"], transport="rccl") == 2 and not calls     # refused, nothing launched
        monkeypatch.undo()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "n_gpus" not in r.stdout and "needs 2 GPUs" in r.stderr


def test_bench_line_names_rccl_only_when_rccl_ran():
    """`rccl_nranks` answers "did RCCL see N ranks?": it may only come from a communicator that IS RCCL (ncclCommCount inside
    plda_comm_describe).  A peer / host / custom transport reports `comm_nranks` and no rccl_* key (round-5 review: a peer line
    printed rccl_nranks: 2, rccl_version: 0)."""
    import importlib
    bench = importlib.import_module("bench")
    ranks = [dict(transport="peer", nranks=2, rank=r, device=0, pci_bus_id="0000:05:00.0", rccl_version=0) for r in range(2)]
    m = bench.describe_ranks(ranks, 1000)
    assert m["transport"] == "peer" and m["comm_nranks"] == 2 and m["distinct_devices"] == 1
    assert not any(k.startswith("rccl") for k in m)
    host = bench.describe_ranks([dict(r, transport="host") for r in ranks])
    assert not any(k.startswith("rccl") for k in host)
    rc = [dict(transport="rccl", nranks=8, rank=r, device=r, pci_bus_id="0000:%02x:00.0" % r, rccl_version=22606) for r in range(8)]
    m = bench.describe_ranks(rc)
    assert m["comm_nranks"] == m["rccl_nranks"] == 8 and m["rccl_version"] == 22606 and m["distinct_devices"] == 8


def test_bench_skewed_labels_are_dense_and_exact():
    """bench.py's `fit_skewed` labelling (C2's rows with unequal speaker counts): exactly N rows, every speaker present, also
    when there are barely more rows than speakers (the --rows overrides of the self-launch tests)."""
    import importlib
    bench = importlib.import_module("bench")
    for n, k in ((100000, 5000), (20000, 5000), (5000, 5000), (6001, 5000), (1200000, 7200)):
        y, nk = bench.skewed_labels(n, k)
        assert y.shape[0] == n and int(nk.sum()) == n and nk.min() >= 1
        assert np.array_equal(np.unique(y), np.arange(k, dtype=y.dtype))
    y, nk = bench.skewed_labels(100000, 5000)
    # BASELINE.md C2's "skewed-n_k variant": counts drawn from [5, 60] and rescaled to the 100k rows -> 3 .. 38, 36 distinct values
    assert len(np.unique(nk)) == 36 and nk.min() == 3 and nk.max() == 38


def test_bench_dump_sample_is_fixed_and_spans_the_matrix():
    """`bench.py --dump-outputs`: the sampled rows / columns depend on the shape alone (two builds compare the same scores),
    hold the first and the last index, are distinct and ascending, and are every index of a small matrix."""
    import importlib
    bench = importlib.import_module("bench")
    for n, k in ((100000, 1024), (1000000, 4096), (4097, 4096), (3, 3)):
        a, b = bench.dump_sample(n, k, 11), bench.dump_sample(n, k, 11)
        assert np.array_equal(a, b) and a.shape == (min(n, k),)
        assert a[0] == 0 and a[-1] == n - 1 and (np.diff(a) > 0).all()
    assert np.array_equal(bench.dump_sample(300, 1024, 11), np.arange(300))
    assert bench.dump_sample(100000, 1024, 11).size * bench.dump_sample(100000, 4096, 12).size * 4 <= 64 << 20


def test_bench_refuses_zero_steps():
    """`--steps` is the number of timed steps and `ms_per_step` divides by it: 0 is refused before anything is set up."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr and not r.stdout
