#!/bin/bash
# usage: tools/build_variant.sh NAME -DMACRO=VALUE … — build/libmeepo_hip_NAME.so with extra compiler flags (A/B runs: MEE_LIB_PATH=build/libmeepo_hip_NAME.so)
# The translation units and their flags, per-file flags included, are the product's own (__graft_entry__.py), so the variant differs from it by the
# extra flags alone.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
rm -rf build/obj_$name   # (objects of a source list that has changed since must not reach the link)
mkdir -p build/obj_$name
# MEE_VARIANT_TU=meepo_apply: the extra flags go to that translation unit only
while IFS=$'\t' read -r f flags; do
  extra=("$@"); if [ -n "$MEE_VARIANT_TU" ] && [ "$MEE_VARIANT_TU" != "$f" ]; then extra=(); fi
  $hipcc $flags "${extra[@]}" -c meepoembedding_amd/csrc/$f.hip -o build/obj_$name/$f.o &
  pids+=($!)
done < <(python3 -c '
import __graft_entry__ as g
for s in g.HIP_SOURCES:
    print(s[:-len(".hip")] + "\t" + " ".join([f for f in g.HIP_FLAGS if f != "-shared"] + g.HIP_FILE_FLAGS.get(s, [])))')
for p in "${pids[@]}"; do wait $p; done   # a failed compile ends the script
$hipcc --offload-arch=gfx950 -shared -fPIC build/obj_$name/*.o -ldl -o build/libmeepo_hip_$name.so
echo build/libmeepo_hip_$name.so
