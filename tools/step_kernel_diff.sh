#!/bin/bash
# Are the step kernels' machine code the same in two builds?  Disassembles the gfx950 code
# object of every dx_step*.o (the generic kernel, every scene specialization, the mid and
# overflow tiers) of two object directories and compares them per unit:
#   cp -r build/obj /tmp/parent_obj        (at the parent commit, after a build)
#   tools/step_kernel_diff.sh /tmp/parent_obj build/obj
set -e
B=/opt/rocm/lib/llvm/bin
T=$(mktemp -d)
dis() {  # object -> disassembly text
  $B/llvm-objcopy --dump-section=.hip_fatbin="$T/fat.bin" "$1"
  $B/clang-offload-bundler --unbundle --type=o --input="$T/fat.bin" \
    --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$T/k.co"
  $B/llvm-objdump -d "$T/k.co" | grep -v "file format"
}
rc=0
for a in "$1"/dx_step*.o; do
  unit=$(basename "$a" | cut -d. -f1)
  b=$(ls "$2"/"$unit".*.o | head -1)
  dis "$a" > "$T/a.s"
  dis "$b" > "$T/b.s"
  if cmp -s "$T/a.s" "$T/b.s"; then
    echo "$unit: identical ($(wc -l < "$T/a.s") lines, $(grep -c '^[0-9a-f]* <' "$T/a.s") symbols)"
  else
    echo "$unit: DIFFERS"
    rc=1
  fi
done
rm -rf "$T"
exit $rc
