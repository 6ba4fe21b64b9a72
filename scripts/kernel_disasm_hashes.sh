#!/bin/bash
set -euo pipefail
# sha256 of the gfx950 disassembly of every KERNEL of one csrc file (addresses, encodings and symbol references stripped), sorted by name: what tells whether a change that
# adds kernels to a file left the others alone (scripts/device_disasm_hashes.sh hashes whole files).  No GPU needed.
# usage: scripts/kernel_disasm_hashes.sh <tree> <out file> [source name, default me.hip]; run on two trees and `join` / `diff` the outputs
R=${ROCM_PATH:-/opt/rocm}; T=$(mktemp -d); SRC=${3:-me.hip}
$R/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-fast-math -ffp-contract=off -Wall -Wno-unused-function --cuda-device-only -c $1/vtm_amd/csrc/$SRC -o $T/a.co
$R/llvm/bin/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$T/a.co --output=$T/a.elf
$R/llvm/bin/llvm-objdump -d $T/a.elf | python3 -c "
import sys,re,hashlib,subprocess
cur=None; h={}
for l in sys.stdin:
    m=re.match(r'^[0-9a-f]+ <(.+)>:',l)
    if m: cur=m.group(1); h[cur]=hashlib.sha256(); continue
    if cur is None: continue
    l=re.sub(r'//.*','',l); l=re.sub(r'<[^>]*>','',l).strip()
    if l: h[cur].update(l.encode()+b'\n')
names=subprocess.run(['c++filt'],input='\n'.join(h),capture_output=True,text=True).stdout.split('\n')
for k,n in zip(h,names):
    n=re.sub(r'\(anonymous namespace\)::','',n); n=re.sub(r'\(.*','',n); n=re.sub(r'^void ','',n)
    print('%-60s %s'%(n[:60],h[k].hexdigest()[:16]))
" | sort > $2
rm -rf $T
