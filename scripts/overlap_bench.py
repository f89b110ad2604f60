"""Overlap-aware diarisation measurements: what the second speaker costs, beside the PARENT commit's
entry points on the same inputs.  Whole calls between HIP events, warm-up, >= 5 timed repetitions, medians, the spread (max -
min) of every arm's repetitions; the shader clock the box reports right after the timed loops is recorded with them.

  der   the inputs of scripts/der_time_bench.py (its recordings, time line, collar 25, the device AHC's labels at threshold 0)
        at its three shapes.  Timed: plda_der_timed_dev; plda_der_timed_ovl_dev with hyp2 = NULL; plda_der_timed_ovl_dev with a
        second label (the recording's next hypothesis speaker) on about 20 % of the speech segments.
  vbx   the inputs of scripts/vbx_bench.py at its three shapes.  Timed: plda_vbx_dev; plda_vbx_top2_dev with both outputs.

Every tree is measured in a process of its own: this script starts itself once per tree with --tree DIR, DIR holding a
plda_amd package with its library built.  --parent-tree DIR names a checkout of the parent commit (git worktree add DIR
HEAD~1, then python -m plda_amd.build in it); in it only the entry points it has are timed.  Without --parent-tree only this
tree is measured and the document says so.  The expectation is parity of this tree's plda_der_timed_ovl_dev (hyp2 = NULL) and
plda_vbx_top2_dev with the parent's plda_der_timed_dev and plda_vbx_dev; `slower_than_parent_spread` is True where the
difference of the medians exceeds the spread of the parent's own repetitions.  The document records, it does not judge.

usage: overlap_bench.py [--arm der,vbx] [--reps 5] [--shapes 2000x100,200x1000,16x4096] [--parent-tree DIR] [--out-dir DIR]
       (default: profiles/; one der_overlap_<R>x<N>.json and one vbx_top2_<R>x<T>.json per shape)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ahc_bench import D, _clock, _timed, synthetic_model  # noqa: E402
from der_bench import recordings  # noqa: E402
from der_time_bench import time_line  # noqa: E402

SECOND = 0.2
COLLAR = 25


def _spread(st):
    st["spread_ms"] = st["max_ms"] - st["min_ms"]
    return st


def der_arm(r, n, reps):
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
    rng = np.random.default_rng(3 * r + n)
    k = np.repeat(ncl, n)
    hyp2 = np.where((rng.random(r * n) < SECOND) & (hyp >= 0) & (k > 1), (hyp + 1) % np.maximum(k, 1), -1).astype(np.int32)
    d = {key: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for key, v in
         (("ts", ts), ("td", td), ("tk", tk), ("ss", start), ("sd", dur), ("hyp", hyp), ("hyp2", hyp2))}
    counts = torch.empty((r, 4), dtype=torch.int64, device=dev)
    mp = torch.empty((r, 64), dtype=torch.int32, device=dev)
    dturns = [d["ts"].data_ptr(), d["td"].data_ptr(), d["tk"].data_ptr()]

    def f_plain():
        eng.der_timed_dev(dturns, toff, d["ss"].data_ptr(), d["sd"].data_ptr(), d["hyp"].data_ptr(), offsets, counts.data_ptr(), mp.data_ptr(),
                          collar=COLLAR)

    def f_ovl(second):
        eng.der_timed_ovl_dev(dturns, toff, d["ss"].data_ptr(), d["sd"].data_ptr(), d["hyp"].data_ptr(),
                              d["hyp2"].data_ptr() if second else None, offsets, counts.data_ptr(), mp.data_ptr(), collar=COLLAR)

    res = {"R": r, "N": n, "collar": COLLAR, "segments": r * n, "turns": int(toff[-1]),
           "second_label_fraction_of_speech_segments": float((hyp2 >= 0).sum() / max(1, (hyp >= 0).sum()))}
    res["der_timed"] = _spread(_timed(f_plain, reps))
    torch.cuda.synchronize()
    res["counts_der_timed"] = counts.sum(0).tolist()
    if hasattr(eng, "der_timed_ovl_dev"):
        res["der_timed_ovl_null"] = _spread(_timed(lambda: f_ovl(False), reps))
        torch.cuda.synchronize()
        res["counts_ovl_null"] = counts.sum(0).tolist()
        res["der_timed_ovl_second"] = _spread(_timed(lambda: f_ovl(True), reps))
        torch.cuda.synchronize()
        res["counts_ovl_second"] = counts.sum(0).tolist()
    res["clock_after"] = _clock()
    del eng
    return res


def vbx_arm(r, t, reps):
    import torch
    import vbx_bench as VB
    import vbx_model as M
    from plda_amd import MPlda, diarize
    dev = torch.device("cuda", 0)
    eng = MPlda(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    eng.set_model(np.zeros(4), np.eye(4), np.ones(4))
    ys, ls = [], []
    for q in range(r):
        y, lab, _, phi = M.generate(t, VB.D, VB.K, VB.S, 10_000 * t + q)
        ys.append(y)
        ls.append(lab)
    offsets = diarize.offsets_of([t] * r)
    dY, dL, dPhi = (torch.from_numpy(a).to(dev) for a in (np.concatenate(ys), np.concatenate(ls), phi))
    oL, oL2 = (torch.empty(r * t, dtype=torch.int32, device=dev) for _ in range(2))
    oP2 = torch.empty(r * t, dtype=torch.float64, device=dev)
    oK = torch.empty(r, dtype=torch.int32, device=dev)
    par = (VB.FA, VB.FB, VB.P, VB.SIGMA, VB.ITERS, float("-inf"))

    def f_plain():
        eng.vbx_dev(dY.data_ptr(), VB.D, dPhi.data_ptr(), dL.data_ptr(), offsets, oL.data_ptr(), oK.data_ptr(), *par)

    def f_top2():
        eng.vbx_top2_dev(dY.data_ptr(), VB.D, dPhi.data_ptr(), dL.data_ptr(), offsets, oL.data_ptr(), oK.data_ptr(), oL2.data_ptr(),
                         oP2.data_ptr(), *par)

    res = {"R": r, "T": t, "D": VB.D, "S": VB.S, "iterations": VB.ITERS, "class": diarize.vbx_plan(eng, t, VB.S, VB.D)}
    res["vbx"] = _spread(_timed(f_plain, reps))
    torch.cuda.synchronize()
    res["labels_sum_vbx"] = int(oL.sum())
    if hasattr(eng, "vbx_top2_dev"):
        res["vbx_top2"] = _spread(_timed(f_top2, reps))
        torch.cuda.synchronize()
        res["labels_sum_top2"] = int(oL.sum())
        res["segments_with_a_second_speaker"] = int((oL2 >= 0).sum())
    res["clock_after"] = _clock()
    del eng
    return res


def child(args):
    """one tree, one arm, every shape: one JSON line per shape on stdout"""
    sys.path.insert(0, args.tree)                       # (before the first import of plda_amd: this tree's package and library)
    import torch
    if not torch.cuda.is_available():
        sys.exit("overlap_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    import plda_amd
    assert os.path.abspath(plda_amd.__file__).startswith(os.path.abspath(args.tree)), plda_amd.__file__
    for shape in args.shapes.split(","):
        r, n = (int(v) for v in shape.split("x"))
        res = (der_arm if args.arm == "der" else vbx_arm)(r, n, args.reps)
        print("RESULT " + json.dumps(res), flush=True)


def run_tree(tree, arm, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--arm", arm, "--reps", str(args.reps), "--shapes", args.shapes]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if out.returncode:
        sys.exit("overlap_bench.py: %s failed in %s (status %d)\n%s" % (arm, tree, out.returncode, out.stderr[-2000:]))
    return [json.loads(ln[7:]) for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]


def compare(mine, parent, new_key, old_key):
    """this tree's new entry beside the parent's old one: the difference of the medians against the parent's own spread"""
    diff = mine[new_key]["median_ms"] - parent[old_key]["median_ms"]
    return {"this": new_key, "parent": old_key, "median_ms_this": mine[new_key]["median_ms"], "median_ms_parent": parent[old_key]["median_ms"],
            "difference_ms": diff, "parent_spread_ms": parent[old_key]["spread_ms"], "ratio": mine[new_key]["median_ms"] / parent[old_key]["median_ms"],
            "slower_than_parent_spread": bool(diff > parent[old_key]["spread_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default="der,vbx")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="2000x100,200x1000,16x4096")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    os.makedirs(args.out_dir, exist_ok=True)
    for arm in args.arm.split(","):
        parent = run_tree(os.path.abspath(args.parent_tree), arm, args) if args.parent_tree else None
        mine = run_tree(ROOT, arm, args)
        for q, res in enumerate(mine):
            doc = {"what": "overlap-aware diarisation, %s arm: this tree beside the parent commit, one process per tree" % arm, "this_tree": res,
                   "parent_tree": parent[q] if parent else "not measured: no --parent-tree"}
            if parent:
                new_key, old_key = ("der_timed_ovl_null", "der_timed") if arm == "der" else ("vbx_top2", "vbx")
                doc["against_parent"] = [compare(res, parent[q], new_key, old_key), compare(res, parent[q], old_key, old_key)]
                if arm == "der":
                    doc["against_parent"].append(compare(res, parent[q], "der_timed_ovl_second", "der_timed"))
                    doc["counts_equal"] = bool(res["counts_ovl_null"] == res["counts_der_timed"] == parent[q]["counts_der_timed"])
                else:
                    doc["labels_equal"] = bool(res["labels_sum_top2"] == res["labels_sum_vbx"] == parent[q]["labels_sum_vbx"])
            name = ("der_overlap_%dx%d.json" if arm == "der" else "vbx_top2_%dx%d.json") % (res["R"], res.get("N", res.get("T")))
            with open(os.path.join(args.out_dir, name), "w") as f:
                json.dump(doc, f, indent=1)
            print(json.dumps({k: doc[k] for k in doc if k != "what"}), flush=True)


if __name__ == "__main__":
    main()
