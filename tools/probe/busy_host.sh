#!/bin/bash
# Do the polled hand-overs still answer in ~20 us when the host is busy (VERDICT r03 weak point 12: 8 ranks = 8 spinning cores next to
# 8 torch processes)?  bench.py alone, then beside N busy-looping processes (N = the box's cores - 1, then 2 x the cores), one GPU.
# Usage (through gpurun): bash tools/probe/busy_host.sh
cores=${ET_BUSY_CORES:-16}  # (the GPU boxes of this pool give a job 16 host cores per GPU: nproc shows the whole host)
OUT=${OUT:-bench_out}  # (where the lines and their logs go)
mkdir -p $OUT
run() {
  python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-extra-workloads > $OUT/busy_$1.json 2> $OUT/busy_$1.err
  python - "$1" "$OUT" <<'PY'
import json,sys
d=json.load(open(f"{sys.argv[2]}/busy_{sys.argv[1]}.json")); p=d["phase_ms"]
print(f"{sys.argv[1]:10s} value {d['value']:7.1f} cold {d['value_cold']:7.1f} | enc_scan {p['enc_scan']:.4f} (K1 -> K4: reduce, the host's code construction, tile scan) | dec_sync - first sweep {p['dec_sync']-p['dec_sync_first']:.4f} | enc {p['enc_total']:.4f} dec {p['dec_total']:.4f} ms")
PY
}
echo "cores: $cores"
run alone
pids=""
for i in $(seq 1 $((cores - 1))); do python3 -c "while True: pass" & pids="$pids $!"; done
sleep 1
run busy_n-1
for i in $(seq 1 $((cores + 1))); do python3 -c "while True: pass" & pids="$pids $!"; done
sleep 1
run busy_2n
kill $pids 2>/dev/null
wait 2>/dev/null
run alone2
