#!/bin/bash
# tools/ab_lib.sh <variant.so> <tool.py> [args]: the tool with the variant library and with the in-tree one, alternating,
# twice each, in one call on one box (devices of the pool differ by up to 10 %: only same-box numbers compare).
# Every run has its own time limit, and the first run that fails ends the script: nothing is started on a device behind
# a fault, an abort or a hang.
set -o pipefail
V="$1"; shift
run() {  # run <label> <library or ""> <tool.py> [args]
  local label="$1" lib="$2" rc; shift 2
  echo "== $label"
  # (grep exits 1 when it lets no line through: only the tool's own status counts)
  PYPERIOD_AMD_LIB="$lib" timeout -k 10 200 python3 "$@" 2>&1 | { grep -v amdgpu.ids || true; }
  rc=$?
  if [ $rc -ne 0 ]; then echo "== $label failed with status $rc: stopping" >&2; exit $rc; fi
}
for i in 1 2; do
  run "variant $(basename "$V")" "$V" "$@"
  run "in-tree" "" "$@"
done
