"""Time-based diarisation error rate measurements: whole calls between HIP events, warm-up, >= 5
timed repetitions, medians; the shader clock the box reports right after the timed loops is recorded with them.

The recordings of scripts/der_bench.py (about 10 planted reference speakers) laid on a time line: segment t of a recording
runs [start, start + dur) back to back; the reference is one turn of the planted speaker per segment, and on about 15 % of the
segments a second speaker talks over it; same-speaker turns are merged (rttm.pack_turns).  Collar 25 ticks, Q = 32 thresholds.
Shapes: R = 2 000 recordings of N = 100 segments, R = 200 of N = 1 000 and R = 16 of N = 4 096.
Timed separately:
  der_timed      plda_der_timed_dev, hypotheses = the device AHC's labels at threshold 0
  sweep_timed    plda_der_timed_sweep_dev on the full merge record, Q = 32
  sweep_segment  plda_der_sweep_dev (K17, the segment form) on the SAME merge record, reference = the planted speaker of
                 every segment: beside sweep_timed it is the cost of atoms over segments
The yardstick is the host, one thread: tests/der_time_model.score_atoms with scipy.optimize.linear_sum_assignment as its
solver, on at most `--host-recordings` recordings, scaled to R; its counts are compared with the device's for equality and
the result is recorded.

No ratio is fixed in advance: the document records, it does not judge.

usage: der_time_bench.py [--reps 5] [--shapes 2000x100,200x1000,16x4096] [--q 32] [--collar 25] [--host-recordings 16]
       [--out-dir DIR]  (default: profiles/; one der_time_<R>x<N>.json per shape)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ahc_bench import D, _clock, _timed, synthetic_model  # noqa: E402
from der_bench import SPEAKERS, host_solver, recordings  # noqa: E402

OVERLAP = 0.15


def time_line(r, n, ref, dur, seed):
    """segment starts (back to back per recording) and the reference turns of every recording, as {recording: [(start, dur,
    speaker)]}: the planted speaker of every segment, and on about OVERLAP of them the next speaker as well"""
    rng = np.random.default_rng(seed)
    start = np.empty(r * n, np.int32)
    turns = {}
    for q in range(r):
        a = q * n
        start[a:a + n] = np.concatenate([[0], np.cumsum(dur[a:a + n])[:-1]])
        k = int(ref[a:a + n].max()) + 1
        over = rng.random(n) < OVERLAP
        tl = []
        for t in range(n):
            g = int(ref[a + t])
            if g < 0:
                continue
            tl.append((int(start[a + t]), int(dur[a + t]), g))
            if over[t] and k > 1:
                tl.append((int(start[a + t]), int(dur[a + t]), (g + 1) % k))
        turns[q] = tl
    return start, turns


def measure(r, n, reps, nq, collar, host_recs):
    import torch
    import der_time_model as T
    from plda_amd import MPlda, der, diarize, rttm
    dev = torch.device("cuda", 0)
    mean, Tm, psi = synthetic_model(D, 15)
    eng = MPlda(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    eng.set_model(mean, Tm, psi)
    vecs, ref, dur = recordings(r, n, psi, 1000 * r + n)
    start, turns_by_rec = time_line(r, n, ref, dur, 7 * r + n)
    (ts, td, tk, toff), _ = rttm.pack_turns(turns_by_rec, list(range(r)))
    offsets = diarize.offsets_of([n] * r)
    hyp, ncl = diarize.ahc_vectors(eng, vecs, offsets, 0.0, None)
    _, _, merges = diarize.ahc_vectors(eng, vecs, offsets, None, 1, return_merges=True)
    cost = merges[2][np.isfinite(merges[2])]
    thresholds = np.ascontiguousarray(-np.quantile(cost, np.linspace(0.5, 0.999, nq)))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         (("ts", ts), ("td", td), ("tk", tk), ("ss", start), ("sd", dur), ("hyp", hyp), ("ref", ref), ("ma", merges[0]), ("mb", merges[1]),
          ("mc", merges[2]))}
    counts = torch.empty((r, 4), dtype=torch.int64, device=dev)
    mp = torch.empty((r, 64), dtype=torch.int32, device=dev)
    scounts = torch.empty((nq, r, 4), dtype=torch.int64, device=dev)
    gcounts = torch.empty((nq, r, 4), dtype=torch.int64, device=dev)
    sncl = torch.empty((nq, r), dtype=torch.int32, device=dev)
    dturns = [d["ts"].data_ptr(), d["td"].data_ptr(), d["tk"].data_ptr()]

    def f_der():
        eng.der_timed_dev(dturns, toff, d["ss"].data_ptr(), d["sd"].data_ptr(), d["hyp"].data_ptr(), offsets, counts.data_ptr(), mp.data_ptr(),
                          collar=collar)

    def f_sweep():
        eng.der_timed_sweep_dev([d["ma"].data_ptr(), d["mb"].data_ptr(), d["mc"].data_ptr()], dturns, toff, d["ss"].data_ptr(),
                                d["sd"].data_ptr(), offsets, thresholds, None, scounts.data_ptr(), sncl.data_ptr(), collar=collar)

    def f_segment():
        eng.der_sweep_dev(d["ma"].data_ptr(), d["mb"].data_ptr(), d["mc"].data_ptr(), offsets, d["ref"].data_ptr(), d["sd"].data_ptr(),
                          thresholds, None, gcounts.data_ptr(), sncl.data_ptr())

    per_rec = np.diff(toff)
    res = {"what": "time-based diarisation error rate: atoms, optimal speaker mapping; sweep of one merge record",
           "R": r, "N": n, "Q": nq, "collar": collar, "segments": r * n, "turns": int(toff[-1]), "reference_speakers": SPEAKERS,
           "overlap_fraction_of_segments": OVERLAP,
           "hypothesis_speakers": {"min": int(ncl.min()), "median": float(np.median(ncl)), "max": int(ncl.max())},
           "event_class_at_median": der.plan_timed(eng, int(np.median(per_rec)), n, 0, collar)}
    res["der_timed"] = _timed(f_der, reps)
    res["sweep_timed"] = _timed(f_sweep, reps)
    res["sweep_segment"] = _timed(f_segment, reps)
    torch.cuda.synchronize()
    res["clock_after"] = _clock()
    res["atoms_over_segments"] = res["sweep_timed"]["median_ms"] / res["sweep_segment"]["median_ms"]
    dc, sc = counts.cpu().numpy(), scounts.cpu().numpy()
    res["pooled_der_at_threshold_0"] = der.pooled(dc)
    res["sweep_pooled_der"] = {"best_q": der.best_index(sc), "min": float(np.nanmin([der.pooled(c) for c in sc]))}

    solve, name = host_solver()
    assign = lambda C: (solve(np.asarray(C, np.int64).reshape(C.shape)) if C.size else 0, None)
    hr = min(r, host_recs)

    def host(labels):
        out = []
        for q in range(hr):
            a, b = int(toff[q]), int(toff[q + 1])
            one = T.rec(ts[a:b], td[a:b], tk[a:b], start[q * n:(q + 1) * n], dur[q * n:(q + 1) * n], labels[q * n:(q + 1) * n])
            out.append(T.score_atoms(one, collar, False, assign)[0])
        return out
    t0 = time.perf_counter()
    hc = host(hyp)
    t_der = time.perf_counter() - t0
    sub_off = offsets[:hr + 1]
    sub_m = tuple(a[:int(sub_off[-1]) - hr] for a in merges)
    t0 = time.perf_counter()
    hs = []
    for thr in thresholds:
        labels, _ = diarize.cut(sub_m, sub_off, float(thr))
        hs.append(host(labels))
    t_sweep = time.perf_counter() - t0
    res["host_baseline"] = {"model": "tests/der_time_model.score_atoms", "solver": name, "threads": 1, "recordings_timed": hr,
                            "der_ms_scaled_to_R": 1e3 * t_der * r / hr, "sweep_ms_scaled_to_R": 1e3 * t_sweep * r / hr,
                            "der_equals_device": bool(np.array_equal(np.asarray(hc), dc[:hr])),
                            "sweep_equals_device": bool(np.array_equal(np.asarray(hs), sc[:, :hr]))}
    res["host_over_device"] = {"der": res["host_baseline"]["der_ms_scaled_to_R"] / res["der_timed"]["median_ms"],
                               "sweep": res["host_baseline"]["sweep_ms_scaled_to_R"] / res["sweep_timed"]["median_ms"]}
    del eng
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="2000x100,200x1000,16x4096")
    ap.add_argument("--q", type=int, default=32)
    ap.add_argument("--collar", type=int, default=25)
    ap.add_argument("--host-recordings", type=int, default=16)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("der_time_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    os.makedirs(args.out_dir, exist_ok=True)
    for shape in args.shapes.split(","):
        r, n = (int(v) for v in shape.split("x"))
        res = measure(r, n, args.reps, args.q, args.collar, args.host_recordings)
        with open(os.path.join(args.out_dir, "der_time_%dx%d.json" % (r, n)), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: res[k] for k in res if k != "what"}), flush=True)


if __name__ == "__main__":
    main()
