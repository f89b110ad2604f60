cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
# usage: bash scripts/gpu_final_check.sh OUTDIR -- the fit probe, the -m gpu suite, smoke and the full C2 bench line
# (bench.py --full: the fit, skewed-fit, z-norm, CPU and D = 1024 figures read below are --full legs), results in OUTDIR
OUT=${1:?usage: bash scripts/gpu_final_check.sh OUTDIR}
mkdir -p "$OUT"
( python scripts/fit_groups_probe.py; PLDA_EM_VARIANT=3 python scripts/fit_groups_probe.py; PLDA_EM_VARIANT=4 python scripts/fit_groups_probe.py ) 2>&1 | grep -v amdgpu.ids > "$OUT/fit_groups.txt"; cat "$OUT/fit_groups.txt"
timeout 2400 python -m pytest tests -m gpu -x -q > "$OUT/gputests.txt" 2>&1
grep -E "passed|failed|error" "$OUT/gputests.txt" | tail -3
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
timeout 900 python bench.py --full > "$OUT/bench_c2_final.json" 2> "$OUT/bench_c2_final.err"; tail -2 "$OUT/bench_c2_final.err"
python - "$OUT/bench_c2_final.json" <<'PY'
import json, sys
r=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print({k:r.get(k) for k in ("value","ms_per_step","fit_em_iters_per_s","fit_skewed_em_iters_per_s")}, r["roofline"]["frac"], r["roofline"].get("traffic"), r["roofline"].get("clock",{}).get("shader_clock_MHz"))
print(r["fit"]["stats_ms"], r["fit"]["em_ms"], r["fit"]["output_ms"], r["fit_skewed"]["em_ms"], r["fit_skewed"]["cpu_oracle"]["gpu_vs_oracle_after_one_iteration"])
print(r.get("znorm_stats",{}).get("ms"), r.get("cpu_baseline",{}).get("value"), r.get("fit_d1024",{}).get("fit_wall_ms"))
PY
