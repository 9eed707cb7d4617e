#!/bin/sh
# Builds tools/step_trace.cpp against the host orchestration of a source tree (sdqn_api_step.hip and sdqn_api_net.hip, and whichever of
# sdqn_api_redo / _reset / _regularize / _dp .hip the tree has, host code only) and prints its grid:
#   tools/step_trace.sh BUILD_DIR [TREE] [--full | --events] > trace.txt
# TREE defaults to this checkout; give another checkout to compare two trees' step orchestration (the tool uses only what api_internal.h
# declares):   tools/step_trace.sh /tmp/a > a.txt; tools/step_trace.sh /tmp/b ../other > b.txt; cmp a.txt b.txt
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$1; shift
TREE=$HERE/..
case "$1" in ""|--*) ;; *) TREE=$1; shift;; esac
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-host-only -O1 -std=c++17 -ffp-contract=off -fno-pie -Wno-unused-value -I$TREE/simple_dqn_amd/csrc"
mkdir -p "$OUT"
OBJS=
for f in sdqn_api_step sdqn_api_net sdqn_api_redo sdqn_api_reset sdqn_api_regularize sdqn_api_dp; do
  [ -f "$TREE/simple_dqn_amd/csrc/$f.hip" ] || continue      # (a tree may have merged the event files into the others)
  $HIPCC $FLAGS -c "$TREE/simple_dqn_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  OBJS="$OBJS $OUT/$f.o"
done
sed "s|../simple_dqn_amd/csrc/api_internal.h|api_internal.h|" "$HERE/step_trace.cpp" > "$OUT/step_trace_main.hip"
$HIPCC $FLAGS -c "$OUT/step_trace_main.hip" -o "$OUT/step_trace_main.o" &
wait
# (everything else these translation units name — the replay, prioritized and generic paths, the rest of the runtime — is never called
# from the entry points the tool drives, so those names may stay unresolved)
${CXX:-g++} -no-pie -Wl,--unresolved-symbols=ignore-all -o "$OUT/step_trace" $OBJS "$OUT/step_trace_main.o"
exec "$OUT/step_trace" "$@"
