#!/bin/bash
# build the library with different -D switches and time the kernels (60 uniform ticks):  scripts/variants.sh -DX,-DY -DZ
# Each variant is the product build (sand_crate_amd/build.py's FLAGS) plus its switches, compiled into
# scratch/variants/ and handed to the timer through $SAND_CRATE_LIB: the tree's own library is not touched.
cd "$(dirname "$0")/.."
base=$(python -c "from sand_crate_amd.build import FLAGS; print(' '.join(FLAGS))") || exit 1
mkdir -p scratch/variants
for v in "$@"; do
  flags=$(echo "$v" | tr ',' ' ')
  lib=scratch/variants/$(echo "$v" | tr -c 'A-Za-z0-9_.=\n-' '_').so
  hipcc $base $flags sand_crate_amd/csrc/sandcrate_hip.hip -o $lib 2> ${lib%.so}.err || { echo "BUILD FAILED $v"; tail -5 ${lib%.so}.err; continue; }
  SAND_CRATE_LIB=$lib python scripts/${TIMER:-quick_time.py} "$v" ${N:-1048576}
done
