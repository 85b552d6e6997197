#!/bin/bash
# Counter passes over the PQ scan alone, counters only (no tracing in the same run), each pass a process of
# its own under a time limit; nothing is started after a pass that failed.
#   scripts/pmc_scan.sh <out dir> [bench args...]      ASL_LIB_PATH selects the library, as in scripts/ab_lib.sh
# -> <out dir>/pmc_summary.txt: per (kernel, grid size) the counters' averages per dispatch
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
out=$1; shift
tag=$(basename "$out")
mkdir -p "$out"
: > "$out/pmc_summary.txt"
pass() {  # name counters...
  name=$1; shift
  rm -rf /tmp/pmc_${tag}_$name
  timeout -k 10 300 rocprofv3 --pmc "$@" --kernel-include-regex "pq_scan" --output-format csv \
     -d /tmp/pmc_${tag}_$name -o x -- python3 bench.py --steps 4 --warmup 1 "${BENCH_ARGS[@]}" \
     > /tmp/pmc_${tag}_$name.log 2>&1 ||
     { rc=$?; echo "[$name] pass failed, exit $rc" >> "$out/pmc_summary.txt"; return $rc; }
  python3 - "$name" /tmp/pmc_${tag}_$name <<'PY' >> "$out/pmc_summary.txt"
import csv, sys, collections, glob
name, root = sys.argv[1], sys.argv[2]
f = glob.glob(f'{root}/**/*counter_collection.csv', recursive=True)
if not f:
    print(name, 'no counter file'); sys.exit(1)
acc = collections.defaultdict(lambda: collections.defaultdict(float)); cnt = collections.Counter(); seen = set()
for r in csv.DictReader(open(f[0])):
    # launches of one kernel at different sizes are different rows: a per-dispatch average must not mix them
    k = r['Kernel_Name'].split('(')[0][:60] + ' grid=' + str(r.get('Grid_Size', '?'))
    acc[k][r['Counter_Name']] += float(r['Counter_Value'])
    key = (k, r['Dispatch_Id'])
    if key not in seen:
        seen.add(key); cnt[k] += 1
for k in acc:
    print(f'[{name}] {k} dispatches={cnt[k]}')
    for c, v in sorted(acc[k].items()):
        print(f'    {c:28s} {v / cnt[k]:16.1f} per dispatch')
PY
}
BENCH_ARGS=("$@")
pass sq SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_WAVE_CYCLES SQ_BUSY_CYCLES &&
pass tcc FETCH_SIZE &&
pass busy VALUBusy GRBM_GUI_ACTIVE &&
cat "$out/pmc_summary.txt"
