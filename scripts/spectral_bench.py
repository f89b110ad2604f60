"""Spectral clustering measurements: whole calls between HIP events, 2 warm-ups, 5 timed
repetitions, medians; the shader clock the box reports right after the timed loops is recorded with them.

The recordings are ahc_bench.py's (seeded, 2 .. 8 planted speakers of unequal counts, D = 128, the score block what the
library's own trials GEMM writes).  Shapes: R = 2 000 recordings of N = 100 segments, R = 200 of N = 1 000 and R = 16 of
N = 2 048, each with P = 1 and with P = 8 pruning values (the default fractions; P = 1 takes the fifth).  Reported per shape:
  matrix       plda_spectral_matrix_dev on the packed blocks in HBM, max_speakers = 16
  eig_share    the share of one further (traced, untimed) call spent inside the eigensolves: the trace's "spectral.eig" spans
               over all "spectral.*" spans.  The trace keeps its first 8 192 spans; a call with more is sampled from its head
               (spans_capped says so).  This is what a batched or an eigenvalues-only solver could win at most.
  ahc          plda_ahc_matrix_dev on the same blocks at threshold 0
  host         scipy.linalg.eigh + the model's k-means (tests/spectral_model.py) on this box's host, one thread where
               threadpoolctl is there to say so, on the first few recordings and scaled to R (host_recordings says how many)
No ratio is fixed in advance: the document records, it does not judge.

usage: spectral_bench.py [--reps 5] [--shapes 2000x100,200x1000,16x2048] [--P 1,8] [--no-host] [--budget-s 0] [--outdir profiles]
       (--budget-s: configurations not started within this many seconds are left out, i.e. stay unmeasured)"""
import argparse
import contextlib
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ahc_bench import D, _clock, _timed, recordings, same_partition, synthetic_model   # noqa: E402

MAX_SPK = 16


def p_table(n, r, P):
    from plda_amd import diarize
    table, _ = diarize.spectral_args(diarize.offsets_of([n] * r), max_speakers=MAX_SPK)
    return table if P == 8 else np.ascontiguousarray(table[:, 4:5])


def host_baseline(blocks, table, n_rec):
    import scipy.linalg
    import spectral_model as M
    try:
        from threadpoolctl import threadpool_limits
        ctx, threads = threadpool_limits(limits=1), 1
    except ImportError:
        ctx, threads = contextlib.nullcontext(), "as configured"
    t_eig = t_rest = 0.0
    labels = []
    with ctx:
        for q in range(n_rec):
            n = blocks[q].shape[0]
            t0 = time.perf_counter()
            c = M.similarity(blocks[q])
            rows, vecs = [], []
            for p in table[q]:
                L, _ = M.laplacian(M.neighbours_fast(c, int(p)))
                t1 = time.perf_counter()
                lam, V = scipy.linalg.eigh(L)
                t_eig += time.perf_counter() - t1
                rows.append(M.eig_row(np.maximum(lam, 0.0), MAX_SPK))
                vecs.append(V)
            pos, _, k_gap, _ = M.choose(rows, n, table[q], MAX_SPK)
            labels.append(M.kmeans(vecs[pos][:, :k_gap])[0])
            t_rest += time.perf_counter() - t0
    return {"recordings": n_rec, "eigh_ms": 1e3 * t_eig, "total_ms": 1e3 * t_rest, "threads": threads,
            "version": __import__("scipy").__version__}, labels


def measure(r, n, P, reps, with_host):
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
    table = p_table(n, r, P)
    dX = torch.from_numpy(vecs).to(dev)
    S = torch.empty(r * n * n, dtype=torch.float32, device=dev)
    for q in range(r):
        x = dX.data_ptr() + q * n * D * 8
        eng.score_matrix_dev(x, None, 1, n, x, n, S.data_ptr() + q * n * n * 4, n)
    t = r * n
    labels = torch.empty(t, dtype=torch.int32, device=dev)
    ncl = torch.empty(r, dtype=torch.int32, device=dev)
    m = t - r
    mg = (torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev),
          torch.empty(m, dtype=torch.float64, device=dev))

    def matrix():
        eng.spectral_matrix_dev(S.data_ptr(), block_off, offsets, table, MAX_SPK, None, 20, labels.data_ptr(), ncl.data_ptr())

    def ahc():
        eng.ahc_matrix_dev(S.data_ptr(), block_off, offsets, 1, 0.0, None, labels.data_ptr(), ncl.data_ptr(), mg[0].data_ptr(),
                           mg[1].data_ptr(), mg[2].data_ptr())

    res = {"what": "spectral clustering with auto-tuned pruning", "host": socket.gethostname(), "R": r, "N": n, "D": D, "P": P,
           "max_speakers": MAX_SPK, "p_row": table[0].tolist(), "plan": diarize.spectral_plan(eng, n, MAX_SPK), "segments": t}
    res["ahc_matrix_form"] = _timed(ahc, reps)
    res["matrix_form"] = _timed(matrix, reps)
    torch.cuda.synchronize()
    lab, k = labels.cpu().numpy().copy(), ncl.cpu().numpy().copy()
    res["clock_after"] = _clock()
    eng.trace_enable(True)
    eng.trace_read(True)
    matrix()
    torch.cuda.synchronize()
    spans = {s["name"]: s for s in eng.trace_read(True) if s["name"].startswith("spectral.")}
    eng.trace_enable(False)
    total = sum(s["ms"] for s in spans.values())
    res["trace_ms"] = {name: s["ms"] for name, s in spans.items()}
    res["spans_capped"] = bool(6 * r * P > 8000)             # (three spans of this file and three of the eigensolver per problem)
    res["eig_share"] = spans["spectral.eig"]["ms"] / total if total > 0 and "spectral.eig" in spans else None
    res["clusters_per_recording"] = {"min": int(k.min()), "median": float(np.median(k)), "max": int(k.max())}
    res["planted_partition_recovered"] = int(sum(same_partition(lab[q * n:(q + 1) * n], spk[q * n:(q + 1) * n]) for q in range(r)))
    res["spectral_over_ahc"] = res["matrix_form"]["median_ms"] / res["ahc_matrix_form"]["median_ms"]
    if with_host:
        n_rec = min(r, max(1, 4000 // n))
        host = S[:n_rec * n * n].cpu().numpy().reshape(n_rec, n, n)
        res["host_eigh_kmeans"], hl = host_baseline(host, table, n_rec)
        res["host_eigh_kmeans"]["scaled_to_R_ms"] = res["host_eigh_kmeans"]["total_ms"] * r / n_rec
        res["host_eigh_kmeans"]["same_partition_as_device"] = int(sum(same_partition(hl[q], lab[q * n:(q + 1) * n]) for q in range(n_rec)))
        res["host_over_matrix_form"] = res["host_eigh_kmeans"]["scaled_to_R_ms"] / res["matrix_form"]["median_ms"]
    del eng
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="2000x100,200x1000,16x2048")
    ap.add_argument("--P", default="1,8")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--budget-s", type=float, default=0.0)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("spectral_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    os.makedirs(args.outdir, exist_ok=True)
    t0 = time.perf_counter()
    for P in (int(v) for v in args.P.split(",")):
        if P not in (1, 8):
            sys.exit("spectral_bench.py: --P takes 1 and 8")
        for shape in args.shapes.split(","):
            r, n = (int(v) for v in shape.split("x"))
            if args.budget_s and time.perf_counter() - t0 > args.budget_s:
                print(json.dumps({"R": r, "N": n, "P": P, "skipped": "time budget: unmeasured"}), flush=True)
                continue
            res = measure(r, n, P, args.reps, not args.no_host)
            with open(os.path.join(args.outdir, "spectral_%dx%d_p%d.json" % (r, n, P)), "w") as f:
                json.dump(res, f, indent=1)
            print(json.dumps({k: res[k] for k in res if k not in ("what", "host")}), flush=True)


if __name__ == "__main__":
    main()
