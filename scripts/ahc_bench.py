"""Speaker clustering measurements: whole calls between HIP events, warm-up, >= 5 timed
repetitions, medians; the shader clock the box reports right after the timed loops is recorded with them.

Seeded block-structured recordings: every recording has 2 .. 8 speakers of unequal segment counts, its segment vectors are a
speaker centre plus unit noise in the model's space, its score block is what the library's own trials GEMM writes for them.
Shapes: R = 2 000 recordings of N = 100 segments (LDS class), R = 200 of N = 1 000 and R = 16 of N = 4 096 (HBM class).
Timed separately, at a score threshold of 0:
  matrix    plda_ahc_matrix_dev on the packed blocks in HBM (count, load, merge and label kernels + the call's one wait)
  operand   plda_score_ahc_dev on the segment vectors (the same + one trials-GEMM call per recording into the slab)
  gemm      those R plda_score_matrix_dev calls alone
The yardstick is the existing alternative: scipy.cluster.hierarchy.linkage(method="average") over the same symmetrised blocks on
this box's host, one thread, the blocks already in host memory (the copy out of the GPU a user would also pay is timed beside
it).  Where scipy's cut at the same height gives the same partition is counted, not asserted: scipy's Lance-Williams means and
the library's sums differ in the last bits, and a tie may break the other way.

No ratio is fixed in advance: the document records, it does not judge.

usage: ahc_bench.py [--reps 5] [--shapes 2000x100,200x1000,16x4096] [--no-scipy] [--out FILE.json]
       (default: profiles/ahc_<R>x<N>.json per shape)"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

D = 128


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def _timed(fn, reps, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return _stats(ms)


def _clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln.lower()][:2]
    except Exception as ex:      # noqa: BLE001 -- the clock line is a note, not a measurement
        return ["not read: %s" % ex]


def synthetic_model(d, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return rng.random(d), q * (0.5 + rng.random(d))[:, None], np.sort(rng.random(d) * 3.0 + 0.05)[::-1].copy()


def recordings(r, n, psi, seed):
    """segment vectors [r * n, D] in the model's space and the planted speaker of each: 2 .. 8 speakers per recording with
    unequal counts, interleaved"""
    rng = np.random.default_rng(seed)
    vecs = np.empty((r * n, D))
    spk = np.empty(r * n, np.int64)
    for q in range(r):
        k = int(rng.integers(2, 9))
        w = rng.random(k) ** 2 + 0.05
        g = rng.choice(k, size=n, p=w / w.sum())
        centres = rng.standard_normal((k, D)) * np.sqrt(psi)
        vecs[q * n:(q + 1) * n] = centres[g] + rng.standard_normal((n, D))
        spk[q * n:(q + 1) * n] = g
    return vecs, spk


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def measure(r, n, reps, with_scipy):
    import torch
    from plda_amd import MPlda, diarize
    dev = torch.device("cuda", 0)
    mean, T, psi = synthetic_model(D, 15)
    eng = MPlda(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    eng.set_model(mean, T, psi)
    vecs, spk = recordings(r, n, psi, 1000 * r + n)
    offsets = diarize.offsets_of([n] * r)
    block_off = diarize.offsets_of([n * n] * r)
    dX = torch.from_numpy(vecs).to(dev)
    S = torch.empty(r * n * n, dtype=torch.float32, device=dev)
    t, m = r * n, r * n - r
    out = {k: torch.empty(t if k == "labels" else r, dtype=torch.int32, device=dev) for k in ("labels", "ncl")}
    mg = (torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev),
          torch.empty(m, dtype=torch.float64, device=dev))

    def gemm():
        for q in range(r):
            x = dX.data_ptr() + q * n * D * 8
            eng.score_matrix_dev(x, None, 1, n, x, n, S.data_ptr() + q * n * n * 4, n)

    def matrix():
        eng.ahc_matrix_dev(S.data_ptr(), block_off, offsets, 1, 0.0, None, out["labels"].data_ptr(), out["ncl"].data_ptr(),
                           mg[0].data_ptr(), mg[1].data_ptr(), mg[2].data_ptr())

    def operand():
        eng.score_ahc_dev(dX.data_ptr(), offsets, 1, 0.0, None, out["labels"].data_ptr(), out["ncl"].data_ptr(),
                          mg[0].data_ptr(), mg[1].data_ptr(), mg[2].data_ptr())

    res = {"what": "speaker clustering, threshold 0", "host": socket.gethostname(), "R": r, "N": n, "D": D,
           "class": diarize.plan(eng, n), "segments": t}
    res["gemm_calls"] = _timed(gemm, reps)
    res["matrix_form"] = _timed(matrix, reps)
    torch.cuda.synchronize()
    labels_m, ncl_m = out["labels"].cpu().numpy().copy(), out["ncl"].cpu().numpy().copy()
    res["operand_form"] = _timed(operand, reps)
    torch.cuda.synchronize()
    labels_o = out["labels"].cpu().numpy()
    res["clock_after"] = _clock()
    res["operand_equals_matrix"] = bool(np.array_equal(labels_m, labels_o))
    res["clusters_per_recording"] = {"min": int(ncl_m.min()), "median": float(np.median(ncl_m)), "max": int(ncl_m.max())}
    res["planted_partition_recovered"] = int(sum(same_partition(labels_m[q * n:(q + 1) * n], spk[q * n:(q + 1) * n]) for q in range(r)))
    if with_scipy:
        from scipy.cluster import hierarchy
        t0 = time.perf_counter()
        host = S.cpu().numpy().reshape(r, n, n)
        t_copy = time.perf_counter() - t0
        iu = np.triu_indices(n, 1)
        t_prep = t_link = 0.0
        agree = 0
        for q in range(r):
            t0 = time.perf_counter()
            c = -((host[q].astype(np.float64) + host[q].T) / 2.0)
            shift = max(0.0, -float(c[iu].min()))
            cond = c[iu] + shift
            t1 = time.perf_counter()
            Z = hierarchy.linkage(cond, method="average")
            t2 = time.perf_counter()
            t_prep += t1 - t0
            t_link += t2 - t1
            agree += same_partition(hierarchy.fcluster(Z, shift, "distance"), labels_m[q * n:(q + 1) * n])
        res["scipy"] = {"linkage_ms": 1e3 * t_link, "symmetrise_condense_ms": 1e3 * t_prep, "device_to_host_ms": 1e3 * t_copy,
                        "threads": 1, "same_partition_as_device": int(agree), "version": __import__("scipy").__version__}
        res["scipy_linkage_over_matrix_form"] = res["scipy"]["linkage_ms"] / res["matrix_form"]["median_ms"]
    del eng
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="2000x100,200x1000,16x4096")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ahc_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    for shape in args.shapes.split(","):
        r, n = (int(v) for v in shape.split("x"))
        res = measure(r, n, args.reps, not args.no_scipy)
        path = args.out or os.path.join(ROOT, "profiles", "ahc_%dx%d.json" % (r, n))
        if args.out and len(args.shapes.split(",")) > 1:
            path = "%s.%dx%d.json" % (os.path.splitext(args.out)[0], r, n)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: res[k] for k in res if k not in ("what", "host")}), flush=True)


if __name__ == "__main__":
    main()
