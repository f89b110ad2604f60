"""Cosine back-end measurements: whole plda_score_matrix_dev calls between device events, every shape
warmed up, >= 9 timed repetitions, medians, the clock read per shape.

Two arms, alternated in one process (cosine, PLDA, cosine again, PLDA again: the spread between two windows of one arm is the
run-to-run spread the other arm is judged against):
  cosine   a handle switched with plda_backend_set(COSINE, D)
  plda     a PLDA handle of the same dimension, uniform count n = 1 (the same GEMM kernel and depth -- asserted)
Per shape also the prep's own time (the "score.pack_operands" span of the library's trace, per call) and its share of HBM
bandwidth from the bytes the shapes imply: (M + Nt) D 8 read + (Mpad + Npad) Kg 4 written.
The trial list: 10^7 pairs through plda_score_pairs on both back-ends (host entry: wall time, the uploads included in both).

usage: cosine_bench.py [--shapes all|small] [--reps 9] [--pairs 10000000] [--out profiles/cosine_<box>.json]
One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from asnorm_bench import _clock, _engine, _timed      # noqa: E402 -- the same harness as the AS-norm figures

SHAPES = [(100000, 100000, 200), (20000, 20000, 192), (20000, 20000, 256), (20000, 20000, 512), (4096, 4096, 200), (256, 256, 200)]
HBM_GBPS = 8000.0      # MI355X peak HBM bandwidth, for the prep's share


def _cosine(D):
    import torch
    from plda_amd import Cosine
    eng = Cosine(D)
    eng.set_stream(torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    return eng


def _prep_ms(eng, call, reps=5):
    import torch
    eng.trace_enable(True)
    eng.trace_read(reset=True)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    spans = {s["name"]: s for s in eng.trace_read(reset=True)}
    eng.trace_enable(False)
    s = spans.get("score.pack_operands")
    return s["ms"] / s["calls"] if s and s["calls"] else None


def matrix(M, Nt, D, reps):
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    U = torch.randn((M, D), dtype=torch.float64, device=dev, generator=g)
    V = torch.randn((Nt, D), dtype=torch.float64, device=dev, generator=g)
    out = torch.empty((M, Nt), dtype=torch.float32, device=dev)
    arms = {"cosine": _cosine(D), "plda": _engine(D)}
    rec = {"M": M, "Nt": Nt, "D": D}
    calls = {k: (lambda e=e: e.score_matrix_dev(U.data_ptr(), None, 1, M, V.data_ptr(), Nt, out.data_ptr(), Nt)) for k, e in arms.items()}
    for rnd in ("", "_again"):
        for k in ("cosine", "plda"):
            rec[k + rnd] = _timed(calls[k], reps)
            rec[k + rnd]["kernel"], rec[k + rnd]["depth"] = arms[k].score_last_kernel(), arms[k].score_last_shape()[2]
    assert rec["cosine"]["kernel"] == rec["plda"]["kernel"] and rec["cosine"]["depth"] == rec["plda"]["depth"] == D, rec
    c, p = [rec["cosine" + r]["median_ms"] for r in ("", "_again")], [rec["plda" + r]["median_ms"] for r in ("", "_again")]
    rec["ratio_cosine_over_plda"] = float(np.mean(c) / np.mean(p))
    lo = min(rec["plda" + r]["min_ms"] for r in ("", "_again"))
    hi = max(rec["plda" + r]["max_ms"] for r in ("", "_again"))
    rec["plda_spread_ms"] = [lo, hi]
    rec["cosine_median_inside_plda_spread"] = bool(all(lo <= x <= hi for x in c))
    Kg = max(-(-D // 8) * 8, 16)
    nbytes = (M + Nt) * D * 8 + (-(-M // 256) * 256 + -(-Nt // 256) * 256) * Kg * 4
    for k in ("cosine", "plda"):
        ms = _prep_ms(arms[k], calls[k])
        rec[k + "_prep_ms"] = ms
        rec[k + "_prep_share_of_hbm"] = nbytes / (ms * 1e-3) / 1e9 / HBM_GBPS if ms else None
    rec["prep_bytes"] = nbytes
    rec["clock"] = _clock()
    return rec


def pairs(P, D=200, M=20000, Nt=20000, reps=3):
    rng = np.random.default_rng(2)
    U, V = rng.standard_normal((M, D)), rng.standard_normal((Nt, D))
    e, t = rng.integers(0, M, P), rng.integers(0, Nt, P)
    rec = {"P": P, "D": D, "M": M, "Nt": Nt, "what": "plda_score_pairs, host entry, wall time"}
    for k, eng in (("cosine", _cosine(D)), ("plda", _engine(D))):
        ms = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            eng.score_trials((np.ones(M, np.int32), U), (1, V), e, t, znorm=False)
            ms.append((time.perf_counter() - t0) * 1e3)
        rec[k] = {"median_ms": float(np.median(ms[1:])), "min_ms": float(min(ms[1:])), "max_ms": float(max(ms[1:])), "reps": reps}
    rec["clock"] = _clock()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=10 ** 7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    box = socket.gethostname().split(".")[0]
    shapes = SHAPES if args.shapes == "all" else SHAPES[1:]
    doc = {"what": "cosine back-end against the PLDA back-end, plda_score_matrix_dev", "box": box, "reps": max(args.reps, 9), "matrix": []}
    for s in shapes:
        doc["matrix"].append(matrix(*s, reps=max(args.reps, 9)))
        print("# %s" % json.dumps(doc["matrix"][-1]), file=sys.stderr, flush=True)
    if args.pairs > 0:
        doc["pairs"] = pairs(args.pairs)
    text = json.dumps(doc, indent=1)
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cosine_%s.json" % box)
    with open(out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
