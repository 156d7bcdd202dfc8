#!/bin/bash
# Build libiunet.so for gfx950 (cross-compiles without a GPU).  build.sh: incremental (sources newer than their objects);
# build.sh --clean: every .hip file from scratch.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/../lib"
mkdir -p "$OUT" "$HERE/obj"
if [ "$1" = "--clean" ]; then rm -f "$HERE"/obj/*.o "$OUT/libiunet.so"; fi      # full rebuild (~30 s on 8 cores): what build() runs
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-result -Wno-int-to-pointer-cast"
pids=()
objs=()                                         # the objects of the sources present (one left behind by a removed source is not linked)
for f in "$HERE"/*.hip; do
  o="$HERE/obj/$(basename "${f%.hip}").o"
  objs+=("$o")
  stale=0
  if [ ! -f "$o" ] || [ "$f" -nt "$o" ]; then stale=1; fi
  for h in "$HERE"/*.h "$HERE/../../include/iunet.h"; do   # any shared header (common.h, launchers.h ..., the public one) newer than the object
    if [ "$h" -nt "$o" ]; then stale=1; fi
  done
  if [ "$stale" = 1 ]; then
    hipcc $FLAGS -c "$f" -o "$o" &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--no-undefined -o "$OUT/libiunet.so" "${objs[@]}"
echo "built $OUT/libiunet.so"
