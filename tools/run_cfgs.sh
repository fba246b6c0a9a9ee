# every BASELINE.json config that fits one GPU, each with the figures of bench.py --full: bash tools/run_cfgs.sh, results under $OUT (default out/)
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-out}
mkdir -p "$OUT"
export OMP_NUM_THREADS=16
show() { python - "$1" <<'PY'
import json,sys
d=json.load(open(sys.argv[1]))
print(sys.argv[1], "%.2f ms/proof (%.2f proofs/s)  unoverlapped %s  api %s  msm %.1f  fft %.1f  create %.2fs  first proof %s s" % (d["ms_per_step"], d["value"], d.get("unoverlapped_ms_per_step"), d.get("api_ms_per_step"), d["msm_ms_per_proof"], d["fft_ms_per_proof"], d["create_s"], d.get("time_to_first_proof_s")), d["config"]["workload"][:60])
PY
}
timeout -k 10 600 python bench.py --full --log-domain 20 --g1-only --steps 3 --warmup 1 --no-cpu-baseline --no-pmc > "$OUT/cfg1.json" 2> "$OUT/cfg1.err" && show "$OUT/cfg1.json" || tail -3 "$OUT/cfg1.err"
timeout -k 10 600 python bench.py --full --log-domain 24 --mix C --steps 3 --warmup 1 --no-cpu-baseline --no-pmc > "$OUT/cfg2c.json" 2> "$OUT/cfg2c.err" && show "$OUT/cfg2c.json" || tail -3 "$OUT/cfg2c.err"
timeout -k 10 600 python bench.py --full --log-domain 20 --steps 3 --warmup 1 --no-cpu-baseline --no-pmc > "$OUT/q20.json" 2> "$OUT/q20.err" && show "$OUT/q20.json" || tail -3 "$OUT/q20.err"
timeout -k 10 600 python bench.py --full --log-domain 22 --steps 3 --warmup 1 --no-cpu-baseline --no-pmc > "$OUT/q22.json" 2> "$OUT/q22.err" && show "$OUT/q22.json" || tail -3 "$OUT/q22.err"
timeout -k 10 600 python bench.py --full --log-domain 22 --ultra --steps 3 --warmup 1 > "$OUT/cfg4.json" 2> "$OUT/cfg4.err" && show "$OUT/cfg4.json" || tail -3 "$OUT/cfg4.err"
( time timeout -k 10 900 python bench.py --full --log-domain 26 --steps 2 --warmup 1 --no-cpu-baseline --no-pmc ) > "$OUT/cfg3.json" 2> "$OUT/cfg3.err" && show "$OUT/cfg3.json" || tail -5 "$OUT/cfg3.err"
tail -4 "$OUT/cfg3.err"
# (round 4) the reference's largest legal domain, 2^27: the piecewise path (ranges above 2^26 scalars) at its own size
( time timeout -k 10 900 python bench.py --full --log-domain 27 --steps 2 --warmup 1 --no-cpu-baseline --no-pmc --host-threads 1 ) > "$OUT/cfg27.json" 2> "$OUT/cfg27.err" && show "$OUT/cfg27.json" || tail -5 "$OUT/cfg27.err"
