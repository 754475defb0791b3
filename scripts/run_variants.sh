#!/bin/bash
# On the GPU box: time every prebuilt variant (scripts/build_variants.sh) with scripts/quick_time.py.
#   N=1048576 scripts/run_variants.sh name1 name2 ...      (no names: every scratch/variants/*.so)
# The timer takes each variant through $SAND_CRATE_LIB (scripts/timing_support.py: use_library): the tree's own
# sand_crate_amd/libsandcrate_hip.so is not touched, so whatever runs next runs the product build.
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd "$(dirname "$0")/.."
names=("$@")
if (( ${#names[@]} == 0 )); then for f in scratch/variants/*.so; do names+=("$(basename $f .so)"); done; fi
for rep in $(seq 1 ${REPS:-1}); do
  for v in "${names[@]}"; do
    SAND_CRATE_LIB=scratch/variants/$v.so python scripts/${TIMER:-quick_time.py} "$v" ${N:-1048576} || echo "FAILED $v"
  done
done
