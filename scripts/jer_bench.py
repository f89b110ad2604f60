"""Jaccard error rate measurements: what the second assignment and the divisions cost, beside the
one-assignment calls on the same inputs and beside the PARENT commit's library.  Whole calls between HIP events, warm-up, >= 5
timed repetitions, medians, the spread (max - min) of every arm's repetitions; the shader clock the box reports right after the
timed loops is recorded with them.

The inputs are those of scripts/overlap_bench.py's der arm (the recordings of scripts/der_time_bench.py: about 10 planted
reference speakers on a time line, collar 25, hypotheses = the device AHC's labels at threshold 0) at its three shapes, with 0 %
and about 20 % second labels.  Timed:
  der_timed_ovl_null / _second        plda_der_timed_ovl_dev (one assignment)
  der_timed_jer_null / _second        plda_der_timed_jer_dev with jmap and spk (two assignments and one division per cell)
  sweep_timed, sweep_timed_jer        plda_der_timed_sweep_dev and plda_der_timed_jer_sweep_dev on the full merge record, Q = 32
The yardstick of the JER call is the host, one thread: tests/jer_model.py (atoms by intervals, weights in Python ints, scipy's
linear_sum_assignment) on at most --host-recordings recordings, scaled to R; its jer is compared with the device's for equality.

Every tree is measured in a process of its own (--tree DIR, DIR holding a plda_amd package with its library built).
--parent-tree DIR names a checkout of the parent commit with its library built; in it only the entry points it has are timed.
The existing entry points are expected inside the parent's run-to-run spread: `slower_than_parent_spread` says where they are
not.  The document records, it does not judge.

usage: jer_bench.py [--reps 5] [--shapes 2000x100,200x1000,16x4096] [--q 32] [--host-recordings 16] [--parent-tree DIR]
       [--out-dir DIR]  (default: profiles/; one jer_<R>x<N>.json per shape)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ahc_bench import D, _clock, _timed, synthetic_model  # noqa: E402
from der_bench import recordings  # noqa: E402
from der_time_bench import time_line  # noqa: E402
from overlap_bench import COLLAR, SECOND, _spread, compare  # noqa: E402


def measure(r, n, reps, nq, host_recs):
    import torch
    from plda_amd import MPlda, diarize, rttm
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
    rng = np.random.default_rng(3 * r + n)
    k = np.repeat(ncl, n)
    hyp2 = np.where((rng.random(r * n) < SECOND) & (hyp >= 0) & (k > 1), (hyp + 1) % np.maximum(k, 1), -1).astype(np.int32)
    d = {key: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for key, v in
         (("ts", ts), ("td", td), ("tk", tk), ("ss", start), ("sd", dur), ("hyp", hyp), ("hyp2", hyp2), ("ma", merges[0]), ("mb", merges[1]),
          ("mc", merges[2]))}
    counts = torch.empty((r, 4), dtype=torch.int64, device=dev)
    mp, jmap = (torch.empty((r, 64), dtype=torch.int32, device=dev) for _ in range(2))
    jer = torch.empty((r, 2), dtype=torch.int64, device=dev)
    spk = torch.empty((r, 64, 3), dtype=torch.int64, device=dev)
    scounts = torch.empty((nq, r, 4), dtype=torch.int64, device=dev)
    sncl = torch.empty((nq, r), dtype=torch.int32, device=dev)
    sjer = torch.empty((nq, r, 2), dtype=torch.int64, device=dev)
    dturns = [d["ts"].data_ptr(), d["td"].data_ptr(), d["tk"].data_ptr()]
    dmerges = [d["ma"].data_ptr(), d["mb"].data_ptr(), d["mc"].data_ptr()]
    second = lambda on: d["hyp2"].data_ptr() if on else None

    def f_ovl(on):
        eng.der_timed_ovl_dev(dturns, toff, d["ss"].data_ptr(), d["sd"].data_ptr(), d["hyp"].data_ptr(), second(on), offsets, counts.data_ptr(),
                              mp.data_ptr(), collar=COLLAR)

    def f_jer(on):
        eng.der_timed_jer_dev(dturns, toff, d["ss"].data_ptr(), d["sd"].data_ptr(), d["hyp"].data_ptr(), second(on), offsets, counts.data_ptr(),
                              jer.data_ptr(), mp.data_ptr(), jmap.data_ptr(), spk.data_ptr(), collar=COLLAR)

    def f_sweep():
        eng.der_timed_sweep_dev(dmerges, dturns, toff, d["ss"].data_ptr(), d["sd"].data_ptr(), offsets, thresholds, None, scounts.data_ptr(),
                                sncl.data_ptr(), collar=COLLAR)

    def f_sweep_jer():
        eng.der_timed_jer_sweep_dev(dmerges, dturns, toff, d["ss"].data_ptr(), d["sd"].data_ptr(), offsets, thresholds, None, scounts.data_ptr(),
                                    sncl.data_ptr(), sjer.data_ptr(), collar=COLLAR)

    res = {"R": r, "N": n, "Q": nq, "collar": COLLAR, "segments": r * n, "turns": int(toff[-1]),
           "hypothesis_speakers": {"min": int(ncl.min()), "median": float(np.median(ncl)), "max": int(ncl.max())},
           "second_label_fraction_of_speech_segments": float((hyp2 >= 0).sum() / max(1, (hyp >= 0).sum()))}
    sums = {}
    for name, on in (("null", False), ("second", True)):
        res["der_timed_ovl_" + name] = _spread(_timed(lambda: f_ovl(on), reps))
        torch.cuda.synchronize()
        sums["ovl_" + name] = counts.sum(0).tolist()
    res["sweep_timed"] = _spread(_timed(f_sweep, reps))
    torch.cuda.synchronize()
    sums["sweep"] = scounts.sum((0, 1)).tolist()
    if hasattr(eng, "der_timed_jer_dev"):
        from plda_amd import der
        import jer_model as J
        import der_overlap_model as O
        for name, on in (("null", False), ("second", True)):
            res["der_timed_jer_" + name] = _spread(_timed(lambda: f_jer(on), reps))
            torch.cuda.synchronize()
            sums["jer_" + name] = counts.sum(0).tolist()
            res["jer_over_der_" + name] = res["der_timed_jer_" + name]["median_ms"] / res["der_timed_ovl_" + name]["median_ms"]
            res["pooled_jer_" + name] = der.pooled_jer(jer.cpu().numpy())
        got = jer.cpu().numpy()                                # (the call with second labels ran last)
        res["sweep_timed_jer"] = _spread(_timed(f_sweep_jer, reps))
        torch.cuda.synchronize()
        sums["sweep_jer"] = scounts.sum((0, 1)).tolist()
        res["jer_over_der_sweep"] = res["sweep_timed_jer"]["median_ms"] / res["sweep_timed"]["median_ms"]
        sj = sjer.cpu().numpy()
        res["sweep_pooled_jer"] = {"best_q": der.best_jer_index(sj), "min": float(np.nanmin([der.pooled_jer(c) for c in sj]))}
        res["counts_equal_the_one_assignment_calls"] = bool(sums["jer_null"] == sums["ovl_null"] and sums["jer_second"] == sums["ovl_second"]
                                                            and sums["sweep_jer"] == sums["sweep"])
        hr = min(r, host_recs)
        t0 = time.perf_counter()
        host = []
        for q in range(hr):
            a, b = int(toff[q]), int(toff[q + 1])
            sl = slice(q * n, (q + 1) * n)
            host.append(J.score(O.rec(ts[a:b], td[a:b], tk[a:b], start[sl], dur[sl], hyp[sl], hyp2[sl]), COLLAR)[1])
        t_host = time.perf_counter() - t0
        res["host_baseline"] = {"model": "tests/jer_model.score (atoms by intervals, Python-int weights, scipy.optimize.linear_sum_assignment)",
                                "threads": 1, "recordings_timed": hr, "jer_ms_scaled_to_R": 1e3 * t_host * r / hr,
                                "jer_equals_device": bool(np.array_equal(np.asarray(host, np.int64), got[:hr]))}
        res["host_over_device"] = res["host_baseline"]["jer_ms_scaled_to_R"] / res["der_timed_jer_second"]["median_ms"]
    res["counts"] = sums
    torch.cuda.synchronize()
    res["clock_after"] = _clock()
    del eng
    return res


def child(args):
    """one tree, every shape: one JSON line per shape on stdout"""
    sys.path.insert(0, args.tree)                       # (before the first import of plda_amd: this tree's package and library)
    import torch
    if not torch.cuda.is_available():
        sys.exit("jer_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    import plda_amd
    assert os.path.abspath(plda_amd.__file__).startswith(os.path.abspath(args.tree)), plda_amd.__file__
    for shape in args.shapes.split(","):
        r, n = (int(v) for v in shape.split("x"))
        print("RESULT " + json.dumps(measure(r, n, args.reps, args.q, args.host_recordings)), flush=True)


def run_tree(tree, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--reps", str(args.reps), "--shapes", args.shapes, "--q", str(args.q),
           "--host-recordings", str(args.host_recordings)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if out.returncode:
        sys.exit("jer_bench.py: failed in %s (status %d)\n%s" % (tree, out.returncode, out.stderr[-2000:]))
    return [json.loads(ln[7:]) for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="2000x100,200x1000,16x4096")
    ap.add_argument("--q", type=int, default=32)
    ap.add_argument("--host-recordings", type=int, default=16)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(args.out_dir, exist_ok=True)
    parent = run_tree(os.path.abspath(args.parent_tree), args) if args.parent_tree else None
    mine = run_tree(ROOT, args)
    for q, res in enumerate(mine):
        doc = {"what": "Jaccard error rate: this tree's one- and two-assignment calls, beside the parent commit's library; one process per tree",
               "this_tree": res, "parent_tree": parent[q] if parent else "not measured: no --parent-tree"}
        if parent:
            doc["against_parent"] = [compare(res, parent[q], key, key) for key in ("der_timed_ovl_null", "der_timed_ovl_second", "sweep_timed")]
            doc["counts_equal_the_parents"] = bool(all(res["counts"][key] == parent[q]["counts"][key] for key in ("ovl_null", "ovl_second", "sweep")))
        with open(os.path.join(args.out_dir, "jer_%dx%d.json" % (res["R"], res["N"])), "w") as f:
            json.dump(doc, f, indent=1)
        print(json.dumps({k: doc[k] for k in doc if k != "what"}), flush=True)


if __name__ == "__main__":
    main()
