#!/bin/sh
# Builds tools/route_trace.cpp against the kernel translation units of a source tree (host code only, -DSDQN_LAUNCH_TRACE) and prints its grid:
#   tools/route_trace.sh BUILD_DIR [TREE] [--default] > routes.txt
# TREE defaults to this checkout; give another checkout (with the same launch.h hook) to compare two trees' launch decisions:
#   diff <(tools/route_trace.sh /tmp/a) <(tools/route_trace.sh /tmp/b ../other)      (tools/route_trace_compare.py ignores launchers that only moved)
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$1; shift
TREE=$HERE/..
case "$1" in ""|--*) ;; *) TREE=$1; shift;; esac
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-host-only -DSDQN_LAUNCH_TRACE -O1 -std=c++17 -ffp-contract=off -fno-pie -I$TREE/simple_dqn_amd/csrc"
mkdir -p "$OUT"
for f in sdqn_kernels sdqn_kernels_ext sdqn_kernels_r3 sdqn_kernels_bt sdqn_kernels_ss; do
  $HIPCC $FLAGS -c "$TREE/simple_dqn_amd/csrc/$f.hip" -o "$OUT/$f.o" &
done
sed "s|../simple_dqn_amd/csrc/kernels.h|kernels.h|" "$HERE/route_trace.cpp" > "$OUT/route_trace_main.hip"
$HIPCC $FLAGS -c "$OUT/route_trace_main.hip" -o "$OUT/route_trace_main.o" &
wait
# (a host-only object still names its code object: nothing registers it here, so the name may stay unresolved)
${CXX:-g++} -no-pie -Wl,--unresolved-symbols=ignore-all -o "$OUT/route_trace" "$OUT"/*.o
exec "$OUT/route_trace" "$@"
