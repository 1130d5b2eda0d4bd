#!/bin/bash
# A/B of the step's epilogue against the parent commit's library on the headline:
#   profiles/tune/ab_epilogue.sh PARENT_LIB OUT.json [tag ...]     (paths relative to the repository root)
# PARENT_LIB: libnfst_hip.so built from the parent commit; tags: variant libraries (python -m nfst_amd.build --variant TAG
# -D...; "product" = the tree's own library).  The parent and every candidate take turns, REPS times each (default 3), on the
# untouched benchmark; every run goes to OUT.json with roofline.kernel_ms and value.  A change is kept only if every one of
# its runs beats every run of the parent in the same call on both figures.  A run that fails ends the script.
cd "$(dirname "$0")/../.."  # the repository root
PARENT=$1; OUT=$2; shift 2
export NFST_TUNING=1
LINES=$(mktemp)
for rep in $(seq 1 ${REPS:-3}); do
  for v in parent "$@"; do
    case $v in
      parent) export NFST_LIB=$PARENT ;;
      product) unset NFST_LIB ;;
      *) export NFST_LIB=nfst_amd/lib/variants/libnfst_hip_$v.so ;;
    esac
    timeout -k 10 180 python bench.py --steps 200 --warmup 20 --no-cpu-baseline --no-aux ${BENCH_ARGS} 2>/dev/null > $LINES.one
    rc=$?
    if [ $rc -ne 0 ]; then echo "$v rep $rep: bench.py ended with status $rc" >&2; exit $rc; fi
    python - $v $rep $LINES.one >> $LINES <<'PY' || exit 1
import json, sys
d = json.loads([l for l in open(sys.argv[3]) if l.startswith("{")][-1])
r = {"variant": sys.argv[1], "rep": int(sys.argv[2]), "kernel_ms": d["roofline"]["kernel_ms"], "value": d["value"],
     "ms_per_step": d.get("ms_per_step"), "kernel_ms_replay": d["roofline"].get("kernel_ms_replay")}
print(json.dumps(r))
sys.stderr.write("%-10s rep %d  kernel %.2f us  value %.4g arcs/s\n" % (r["variant"], r["rep"], r["kernel_ms"] * 1e3, r["value"]))
PY
  done
done
python - $LINES $OUT <<'PY'
import json, sys
runs = [json.loads(l) for l in open(sys.argv[1])]
by = {}
for r in runs:
    by.setdefault(r["variant"], []).append(r)
par = by["parent"]
summary = {}
for v, rs in by.items():
    k = [r["kernel_ms"] * 1e3 for r in rs]
    val = [r["value"] for r in rs]
    s = {"kernel_us": [round(x, 3) for x in k], "value": val}
    if v != "parent":
        s["beats_parent_in_every_run"] = bool(max(k) < min(r["kernel_ms"] * 1e3 for r in par) and min(val) > max(r["value"] for r in par))
    summary[v] = s
json.dump({"command": "python bench.py --steps 200 --warmup 20 --no-cpu-baseline --no-aux", "rule": "kept only if every run beats every run of the parent on kernel_ms and value",
           "summary": summary, "runs": runs}, open(sys.argv[2], "w"), indent=1)
for v, s in summary.items():
    print(v, s["kernel_us"], ["%.4g" % x for x in s["value"]], s.get("beats_parent_in_every_run", ""))
PY
