#!/bin/bash
# sha256 of the gfx950 disassembly of every csrc/*.hip of one or more source trees, side by side (no GPU needed): a host-only change leaves every row "same".
# The ELF itself differs between two compiles in the __hip_cuid_<hash> symbol name, so the disassembly (minus its file-name header) is what gets hashed.
# A file without device code (ctx.hip, driver.hip) disassembles to nothing: its hash is that of the empty input, e3b0c44298fc1c14.
# usage: git worktree add /tmp/parent HEAD~1 && scripts/device_disasm_hashes.sh /tmp/parent . > profiles/<tag>_device_disasm_hashes.txt
ROCM=${ROCM_PATH:-/opt/rocm}
T=$(mktemp -d); trap 'rm -rf $T' EXIT
hash_one() {   # <tree> <tree index> <file>: writes $T/<index>.<file>
  o=$T/$2.$3
  $ROCM/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-fast-math -ffp-contract=off -Wall -Wno-unused-function --cuda-device-only -c $1/vtm_amd/csrc/$3 -o $o.co 2> /dev/null &&
  $ROCM/llvm/bin/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$o.co --output=$o.elf &&
  $ROCM/llvm/bin/llvm-objdump -d $o.elf | tail -n +3 | sha256sum | cut -c1-16 > $o || echo FAILED > $o
}
export -f hash_one; export ROCM T
files=$(cd ${@: -1}/vtm_amd/csrc && ls *.hip)
i=0; for t in "$@"; do for f in $files; do echo "$t $i $f"; done; i=$(( i + 1 )); done | xargs -P ${JOBS:-8} -L 1 bash -c 'hash_one $0 $1 $2'
printf '%-16s' file; for t in "$@"; do printf ' %-16s' "$(git -C $t rev-parse --short HEAD)$(git -C $t diff --quiet HEAD || echo +)"; done; echo
for f in $files; do
  printf '%-16s' $f; i=0; for t in "$@"; do printf ' %-16s' $(cat $T/$i.$f); i=$(( i + 1 )); done
  [ $(cat $T/*.$f | sort -u | wc -l) = 1 ] && echo ' same' || echo ' DIFFERENT'
done
