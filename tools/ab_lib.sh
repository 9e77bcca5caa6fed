#!/bin/bash
# Build a variant of libgf_hip.so with extra compiler flags (here, no GPU needed) for an A/B run on the GPU box:
#   tools/ab_lib.sh <name> "<flags>" [sources to rebuild ...]   ->  graphflow_amd/csrc/libgf_hip_<name>.so   (select with GF_HIP_LIBRARY=<path>)
# Every other object is the tree's own (run `make` first); the list of objects is the Makefile's SRCS, plus its two host objects.
set -e
NAME=$1; FLAGS=$2; shift 2
cd "$(dirname "$0")/../graphflow_amd/csrc"
SRCS=$(sed -n 's/^SRCS *= *//p' Makefile)
[ -n "$SRCS" ] || { echo "no SRCS in $(pwd)/Makefile" >&2; exit 1; }
for r in "$@"; do
  case " $SRCS " in *" $r.hip "*) ;; *) echo "$r.hip is not in the Makefile's SRCS" >&2; exit 1 ;; esac
done
OBJS=""
for src in $SRCS; do
  f=${src%.hip}
  o=$f.o
  for r in "$@"; do
    if [ "$r" = "$f" ]; then o=/tmp/ab_${NAME}_$f.o; /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../../include $FLAGS -c $f.hip -o $o; fi
  done
  OBJS="$OBJS $o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o libgf_hip_$NAME.so $OBJS smp_prep.o smp_config.o -ldl -lpthread
ls -la libgf_hip_$NAME.so
