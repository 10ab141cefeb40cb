#!/bin/bash
# Development aid: a variant build of libagpl.so for same-box A/B runs (tools/kbench.py, tools/time_update.py, tools/bench_with_lib.py: AGPL_LIB_AB=<name>):
#   tools/build_variant.sh <suffix> <file.hip> "<extra -D flags>"   ->  augmentedgplikelihoods.jl_amd/libagpl_<suffix>.so
# The other objects are the regular build's (run make first).  File list and per-file flags are the Makefile's own: its commands
# for the file's object and for the link, with the output names replaced.
set -e
cd "$(dirname "$0")/../augmentedgplikelihoods.jl_amd/csrc"
SUF=$1; SRC=$2; FLAGS=$3; OBJ=${SRC%.hip}.o
CC=$(make -n -B "$OBJ" | grep -- " -c $SRC ")
LINK=$(make -n -B ../libagpl.so | grep -- " -shared ")
${CC/-o $OBJ/-o variant_$SUF.o} $FLAGS
LINK=${LINK/-o ..\/libagpl.so/-o ../libagpl_$SUF.so}
${LINK/ $OBJ / variant_$SUF.o }
echo built ../libagpl_$SUF.so
