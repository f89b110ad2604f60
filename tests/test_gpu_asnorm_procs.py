"""GPU: plda_cohort_stats_sharded_dev between PROCESSES -- two ranks on the one GPU of the test box, the handle's collective
table backed by the host transport (gloo between the processes), in the style of tests/test_gpu_comm_procs.py.  Every rank
passes all rows and the whole cohort, scores its contiguous slab and ends, after one all-gather of the two result vectors,
with all R results: bit-identical to the single-rank call and between the ranks."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _set_model(eng, d, seed=3):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    eng.set_model(rng.random(d), q * (1.0 + rng.random(d))[:, None], np.sort(rng.random(d) * 4.0 + 0.05)[::-1].copy())


def _rank_main(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from plda_amd import MPlda
        from plda_amd.sharding import cohort_stats_sharded, init_comm
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        ok = {}
        eng, one = MPlda(0), MPlda(0)                  # `one`: the single-rank reference, no communicator
        assert init_comm(eng, transport="host") == (world, rank)
        st = torch.cuda.current_stream(dev).cuda_stream
        eng.set_stream(st); one.set_stream(st)
        d, r, nc, K = 48, 777, 1300, 100               # 777 rows: uneven slabs
        _set_model(eng, d); _set_model(one, d)
        rng = np.random.default_rng(8)                 # same data on every rank (replicated inputs)
        X = torch.from_numpy(rng.standard_normal((r, d))).to(dev)
        Cv = torch.from_numpy(rng.standard_normal((nc, d))).to(dev)
        for tag, n in (("uniform", None), ("mixed", torch.from_numpy(rng.integers(1, 4, r).astype(np.int32)).to(dev))):
            ref = torch.empty((2, r), dtype=torch.float64, device=dev)
            one.cohort_stats_dev(X.data_ptr(), n.data_ptr() if n is not None else None, 0 if n is not None else 2, r, Cv.data_ptr(), nc, K,
                                 ref[0].data_ptr(), ref[1].data_ptr())
            mean, std = cohort_stats_sharded(eng, X, n, Cv, K, n_uniform=0 if n is not None else 2)
            torch.cuda.synchronize()
            got = torch.stack([mean, std])
            ok[tag] = bool(torch.equal(got, ref))
            every = [None] * world
            dist.all_gather_object(every, got.cpu().numpy().tobytes())
            ok[tag + "_replicas"] = all(z == every[0] for z in every)
        eng.comm_destroy()
        q.put((rank, ok))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:      # noqa: BLE001 -- report instead of hanging the peer's collectives
        import traceback
        q.put((rank, {"exception: %s" % traceback.format_exc(): False}))
        raise e


def test_cohort_stats_sharded_between_two_processes():
    import multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 41500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=600) for _ in procs), key=lambda x: x[0])
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    for rank, ok in res:
        bad = [k for k, v in ok.items() if not v]
        assert not bad, (rank, bad)
    assert [p.exitcode for p in procs] == [0] * world
