set -e
OUT=${OUT:-out}
mkdir -p "$OUT"
run() { # name, env...
  name=$1; shift
  env "$@" timeout -k 10 200 python bench.py --full --dev-library --no-cpu-baseline > "$OUT/ab_$name.json" 2> "$OUT/ab_$name.err"
  python - "$name" "$OUT" <<'PY'
import json, sys
d = json.load(open(f"{sys.argv[2]}/ab_{sys.argv[1]}.json"))
k = d["kernel_ms_per_step"]
print(sys.argv[1], "value", round(d["value"], 2), "ms", round(d["ms_per_step"],3), "chain", round(k["chain"], 3), "err", d["error_after_one_iteration"])
PY
}
if [ -n "$TESTS" ]; then
timeout -k 10 600 python -m pytest $TESTS -m gpu -x -q > "$OUT/tests.log" 2>&1 || { tail -30 "$OUT/tests.log"; exit 1; }
tail -3 "$OUT/tests.log"
fi
for v in "$@"; do
  run "$(echo $v | tr '= ' '__')" $v
done
