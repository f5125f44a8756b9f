#!/bin/bash
# Store-policy probe (profiles/store_policy_probe.txt): one GPU run of `cold_stream_probe.bin store`.
#   bash tools/probe/store_policy_probe.sh [out.txt]
# The binary is built beforehand (no GPU needed):
#   hipcc --offload-arch=gfx950 -O3 -o tools/probe/cold_stream_probe.bin tools/probe/cold_stream_probe.hip
set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
out=${1:-profiles/store_policy_probe.txt}
test -x tools/probe/cold_stream_probe.bin || { echo "build tools/probe/cold_stream_probe.bin first (see the header of this script)"; exit 1; }
mkdir -p "$(dirname "$out")" &&
timeout -k 10 240 tools/probe/cold_stream_probe.bin store > "$out.tmp" &&
mv "$out.tmp" "$out" &&
cat "$out"
