"""Trial-key partition measurements: whole calls between HIP events, warm-up, >= 5 timed repetitions with the
arms ALTERNATED (partition, yardstick, partition, ...), medians; the shader clock the box reports right after the timed loops
is recorded with them.

Cases, per size M x Nt (seeded fp32 scores made on the device, 1 000 speakers):
  one       one bucket, every pair a trial
  four      2 x 2 codes, every pair a trial, four buckets
  five_pc   20 x 20 codes, a pair is a trial iff its codes are equal: about 5 % of the pairs, one bucket
and at the largest size the operand form (plda_score_partition_dev, D = 128) with the 5 % key.
Beside every case, taken in the same run: plda_eer_matrix_dev on the same matrix (a pure 4 B / trial read), and on the
20 000 x 20 000 matrix stock torch `S[mask]` per list -- what users do now (the masks are built outside the timed region).
Achieved bytes / s counts 4 B per read trial plus 8 B (one read by the consumer's later pass is NOT counted: 4 B read here +
4 B written) per selected trial.

No ratio is fixed in advance: the document records, it does not judge.

usage: partition_bench.py [--reps 5] [--sizes 20000,100000] [--out FILE.json]   (default: profiles/partition_<M>x<Nt>.json)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ahc_bench import _clock, _stats, synthetic_model  # noqa: E402

D = 128
SPEAKERS = 1000
TORCH_MASK_MAX = 20000


def keys(m, nt, seed):
    from plda_amd import trialkey as TK
    rng = np.random.default_rng(seed)
    e2, t2 = rng.integers(0, 2, m), rng.integers(0, 2, nt)
    e20, t20 = rng.integers(0, 20, m), rng.integers(0, 20, nt)
    return {"one": TK.TrialKey(m, nt, "all"),
            "four": TK.TrialKey(e2, t2, {(a, b): "%d%d" % (a, b) for a in (0, 1) for b in (0, 1)}),
            "five_pc": TK.TrialKey(e20, t20, {(c, c): "same" for c in range(20)})}


def alternated(fns, reps, warmup=2):
    """{name: stats of ms}: the arms take turns inside every repetition"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: _stats(v) for k, v in ms.items()}


def measure(n, reps, with_operands):
    import torch
    from plda_amd import MPlda, eer
    from plda_amd import trialkey as TK
    dev = torch.device("cuda", 0)
    eng = MPlda(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    m = nt = n
    rng = np.random.default_rng(n)
    es, ts = rng.integers(0, SPEAKERS, m).astype(np.int64), rng.integers(0, SPEAKERS, nt).astype(np.int64)
    des, dts = torch.from_numpy(es).to(dev), torch.from_numpy(ts).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    S = torch.empty((m, nt), dtype=torch.float32, device=dev)
    for r0 in range(0, m, 4096):
        S[r0:r0 + 4096].normal_(generator=gen)
    res = {"what": "trial-key partition: per-(bucket, class) score lists of a resident trials matrix", "M": m, "Nt": nt, "cases": {}}

    def f_eer():
        eer.eer_from_matrix_dev(eng, S.data_ptr(), nt, m, nt, des.data_ptr(), dts.data_ptr())

    for name, key in keys(m, nt, n).items():
        rec = key.plan(es, ts)[0]
        selected = int(rec["total"].sum())
        holder = {}

        def f_part(key=key):
            holder["part"] = TK.partition_matrix_dev(eng, key, S, des, dts)

        t = alternated({"partition": f_part, "eer_matrix": f_eer}, reps)
        nbytes = 8 * selected + 4 * m * nt
        case = {"buckets": key.n_buckets, "selected": selected, "selected_fraction": selected / (m * nt), "partition": t["partition"],
                "eer_matrix": t["eer_matrix"], "bytes": nbytes, "achieved_GB_per_s": nbytes / (1e6 * t["partition"]["median_ms"]),
                "eer_GB_per_s": 4 * m * nt / (1e6 * t["eer_matrix"]["median_ms"])}
        if n <= TORCH_MASK_MAX:
            bucket = torch.from_numpy(key.table.astype(np.int64)).to(dev)[torch.from_numpy(key.enrol_code.astype(np.int64)).to(dev)[:, None],
                                                                         torch.from_numpy(key.test_code.astype(np.int64)).to(dev)[None, :]]
            tgt = des[:, None] == dts[None, :]
            masks = [(bucket == b) & (tgt == bool(c)) for b in range(key.n_buckets) for c in (0, 1)]
            del bucket, tgt

            def f_torch():
                holder["lists"] = [S[mk] for mk in masks]

            case["torch_masked_select"] = alternated({"torch": f_torch}, reps)["torch"]
            part = holder["part"]
            eng.synchronize()
            # (torch's order is row-major, the partition's strip-major: the same multiset per list)
            case["torch_lists_have_the_partitions_sizes"] = bool(
                [int(x.shape[0]) for x in holder["lists"]] == [int(part.counts[b][c]) for b in range(key.n_buckets) for c in (0, 1)])
            del masks
            holder.pop("lists", None)
        holder.clear()
        res["cases"][name] = case
        print(json.dumps({name: case}), flush=True)
    if with_operands:
        del S
        torch.cuda.empty_cache()
        mean, T, psi = synthetic_model(D, 15)
        eng.set_model(mean, T, psi)
        U = torch.from_numpy(rng.standard_normal((m, D))).to(dev)
        V = torch.from_numpy(rng.standard_normal((nt, D))).to(dev)
        key = keys(m, nt, n)["five_pc"]
        holder = {}

        def f_opr():
            holder["part"] = TK.partition_from_operands_dev(eng, key, U, None, 1, V, des, dts)

        def f_eer_opr():
            eer.eer_from_operands_dev(eng, U.data_ptr(), None, 1, m, V.data_ptr(), nt, des.data_ptr(), dts.data_ptr())

        t = alternated({"score_partition": f_opr, "score_eer": f_eer_opr}, reps)
        res["operands_five_pc"] = {"D": D, "score_partition": t["score_partition"], "score_eer": t["score_eer"],
                                   "selected": int(key.plan(es, ts)[0]["total"].sum())}
        print(json.dumps({"operands_five_pc": res["operands_five_pc"]}), flush=True)
    torch.cuda.synchronize()
    res["clock_after"] = _clock()
    del eng
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="20000,100000")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("partition_bench.py: no GPU -- these are measurements, there is nothing to fall back to")
    sizes = [int(v) for v in args.sizes.split(",")]
    for n in sizes:
        res = measure(n, args.reps, with_operands=(n == max(sizes)))
        path = args.out or os.path.join(ROOT, "profiles", "partition_%dx%d.json" % (n, n))
        if args.out and len(sizes) > 1:
            path = "%s.%dx%d.json" % (os.path.splitext(args.out)[0], n, n)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
