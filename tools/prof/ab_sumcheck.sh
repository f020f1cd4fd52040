#!/bin/bash
# A/B of the sumcheck prover between two builds of the library in one GPU session:
#   bash tools/prof/ab_sumcheck.sh <library A (e.g. the parent commit's)> <library B> <out.jsonl> [samples]
# For every workload (n = 2^20 and 2^22; degree 3 x 2 products and degree 5 x 1 product; both
# fields) tools/sumcheck_bench.py runs as A, B, A, B: the two A runs show the spread a build has
# against itself, which is what a difference between A and B has to exceed to mean anything.
A=$1; B=$2; OUT=$3; SAMPLES=${4:-5}
cd "$(dirname "$0")/../.." || exit 1
: > "$OUT"
for shape in "1048576 3 2" "4194304 3 2" "1048576 5 1" "4194304 5 1"; do
  for lib in "$A" "$B" "$A" "$B"; do
    BLITZAR_AMD_LIB=$lib timeout -k 10 300 python tools/sumcheck_bench.py $shape "$SAMPLES" \
      | grep '^{' >> "$OUT" || exit 1
  done
done
python - "$OUT" <<'PY'
import json, sys
for line in open(sys.argv[1]):
    r = json.loads(line)
    for f, v in r["fields"].items():
        dev = v["device"]["median_ms"] if isinstance(v["device"], dict) else "absent"
        print(r["n"], r["degree"], r["num_products"], "field", f, r["library"].split("/lib/")[-1],
              "host", v["host"]["median_ms"], "device", dev, "callback", v["callback_ms"])
PY
