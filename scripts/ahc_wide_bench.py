"""Corpus-scale clustering measurements: whole calls of plda_ahc_wide_matrix_dev between HIP events, warm-up,
timed repetitions, medians; the shader clock the box reports right after the timed loops is recorded with them.

Two block families, made on the device, at a score threshold of 0:
  planted    16 groups of unequal sizes, +1 inside and -1 across, interleaved: N - 16 merges, the heaviest tie load
  gaussian   independent standard normal scores: the run stops where the best pair's average score falls below 0
Shapes: N = 4096, 8192, 16384 and 32768.  Per call the record holds the merges made, so a time per step can be read off.

The yardsticks:
  N = 4096   the one-workgroup HBM class (plda_ahc_matrix_dev) on the same block, the two arms alternated call by call
  N = 8192   scipy.cluster.hierarchy.linkage(method="average") on this box's host, one thread, the block already in host memory
             and symmetrised (the copy out of the GPU a user would also pay is timed beside it)

No ratio is fixed in advance: the document records, it does not judge.

usage: ahc_wide_bench.py [--reps 5] [--sizes 4096,8192,16384,32768] [--no-scipy] [--out FILE.json]
       (default: profiles/ahc_wide_<N>.json per size)"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def _event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _timed(fns, reps, warmup=1):
    """the arms of `fns` alternated call by call -> one stats record per arm"""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(_event_ms(fn))
    return [_stats(m) for m in ms]


def _clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln.lower()][:2]
    except Exception as ex:      # noqa: BLE001 -- the clock line is a note, not a measurement
        return ["not read: %s" % ex]


def blocks(n, dev):
    """{"planted": S, "gaussian": S} fp32 [n, n] on the device, seeded by n"""
    import torch
    rng = np.random.default_rng(n)
    w = rng.random(16) + 0.2
    sizes = np.maximum(1, np.floor(w / w.sum() * n).astype(np.int64))
    sizes[0] += n - sizes.sum()
    g = torch.from_numpy(rng.permutation(np.repeat(np.arange(16), sizes))).to(dev)
    planted = torch.where(g[:, None] == g[None, :], 1.0, -1.0).to(torch.float32).contiguous()
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    return {"planted": planted, "gaussian": torch.randn((n, n), generator=gen, device=dev, dtype=torch.float32)}


def measure(n, reps, with_scipy):
    import torch
    from plda_amd import MPlda, diarize
    dev = torch.device("cuda", 0)
    eng = MPlda(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    labels, ncl = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    mg = (torch.empty(n - 1, dtype=torch.int32, device=dev), torch.empty(n - 1, dtype=torch.int32, device=dev),
          torch.empty(n - 1, dtype=torch.float64, device=dev))
    res = {"what": "corpus-scale clustering (wide class), threshold 0, whole calls", "host": socket.gethostname(), "N": n,
           "plan": diarize.plan_wide(eng, n), "families": {}}
    for family, S in blocks(n, dev).items():
        def wide(S=S):
            eng.ahc_wide_matrix_dev(S.data_ptr(), n, n, 1, 0.0, 1, labels.data_ptr(), ncl.data_ptr(), mg[0].data_ptr(), mg[1].data_ptr(),
                                    mg[2].data_ptr())

        arms = [wide]
        if n <= diarize.AHC_MAX:
            block_off, offsets = diarize.offsets_of([n * n]), diarize.offsets_of([n])
            l2, k2 = torch.empty_like(labels), torch.empty_like(ncl)
            m2 = tuple(torch.empty_like(t) for t in mg)

            def one_workgroup(S=S):
                eng.ahc_matrix_dev(S.data_ptr(), block_off, offsets, 1, 0.0, None, l2.data_ptr(), k2.data_ptr(), m2[0].data_ptr(),
                                   m2[1].data_ptr(), m2[2].data_ptr())

            arms.append(one_workgroup)
        stats = _timed(arms, reps)
        torch.cuda.synchronize()
        merges = int((mg[0] >= 0).sum().item())
        rec = {"wide": stats[0], "merges": merges, "clusters": int(ncl.item()),
               "wide_us_per_step": 1e3 * stats[0]["median_ms"] / max(merges, 1)}
        if len(arms) > 1:
            rec["one_workgroup_hbm_class"] = stats[1]
            rec["wide_over_one_workgroup"] = stats[0]["median_ms"] / stats[1]["median_ms"]
            rec["records_equal"] = bool(all(torch.equal(a, b) for a, b in zip((labels, ncl) + mg, (l2, k2) + m2)))
        if with_scipy and n == 8192:
            from scipy.cluster import hierarchy
            t0 = time.perf_counter()
            host = S.cpu().numpy()
            t_copy = time.perf_counter() - t0
            t0 = time.perf_counter()
            c = -((host.astype(np.float64) + host.T) / 2.0)
            iu = np.triu_indices(n, 1)
            cond = c[iu]
            cond = cond + max(0.0, -float(cond.min()))
            t1 = time.perf_counter()
            hierarchy.linkage(cond, method="average")
            t2 = time.perf_counter()
            rec["scipy"] = {"linkage_ms": 1e3 * (t2 - t1), "symmetrise_condense_ms": 1e3 * (t1 - t0), "device_to_host_ms": 1e3 * t_copy,
                            "threads": 1, "version": __import__("scipy").__version__,
                            "note": "linkage builds the full tree (N - 1 merges); the device run stops at the threshold"}
            rec["scipy_linkage_over_wide"] = rec["scipy"]["linkage_ms"] / stats[0]["median_ms"]
        res["families"][family] = rec
    res["clock_after"] = _clock()
    del eng
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="4096,8192,16384,32768")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ahc_wide_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    sizes = [int(v) for v in args.sizes.split(",")]
    for n in sizes:
        res = measure(n, args.reps, not args.no_scipy)
        path = args.out or os.path.join(ROOT, "profiles", "ahc_wide_%d.json" % n)
        if args.out and len(sizes) > 1:
            path = "%s.%d.json" % (os.path.splitext(args.out)[0], n)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: res[k] for k in res if k not in ("what", "host")}), flush=True)


if __name__ == "__main__":
    main()
