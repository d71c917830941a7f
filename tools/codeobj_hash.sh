#!/bin/bash
# sha256 of the product gfx950 code object built from csum_kernels.hip and what it includes under csrc/ (default:
# the working tree's; or a git revision's with REV=<rev>), with a fixed -cuid so that two builds of the same source
# are byte-identical. Used to show that a source change is code-neutral (e.g. the WaveStamps hook, DESIGN.md §7 step
# 76).
#   bash tools/codeobj_hash.sh            # working tree
#   REV=HEAD bash tools/codeobj_hash.sh   # a revision
# KERNELS=1 prints one "symbol sha256" line per kernel instead, sorted by symbol: the hash of the kernel's
# disassembly without addresses and encodings. Branch operands are relative, so a kernel's hash does not depend on
# where it lands in the object; use it where a change reorders or renames kernels.
# DUMP=<dir> also leaves each kernel's normalised disassembly there as <symbol>.s, to diff one against another.
#   KERNELS=1 bash tools/codeobj_hash.sh | diff profiles/refactor_kernels_parent.txt -
set -eu
cd "$(dirname "$0")/.."
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
csrc=$PWD/network-stack_amd/csrc
probes=$PWD/tools/probes
if [ -n "${REV:-}" ]; then
    git archive "$REV" network-stack_amd/csrc tools/probes/wave_stamps.h | tar -x -C "$tmp"
    csrc=$tmp/network-stack_amd/csrc
    probes=$tmp/tools/probes
fi
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -I"$PWD/include" -I"$csrc" -I"$probes" --offload-arch=gfx950 \
    -munsafe-fp-atomics -cuid=nsx --cuda-device-only -c "$csrc/csum_kernels.hip" -o "$tmp/d.o"
/opt/rocm/lib/llvm/bin/clang-offload-bundler --unbundle --type=o --input="$tmp/d.o" \
    --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$tmp/d.co"
if [ -z "${KERNELS:-}" ]; then sha256sum "$tmp/d.co" | cut -d' ' -f1; exit; fi
mkdir "$tmp/k"
/opt/rocm/lib/llvm/bin/llvm-objdump -d "$tmp/d.co" | awk -v dir="$tmp/k" '
    /^[0-9a-f]+ <.*>:$/ { if (f != "") close(f); f = dir "/" substr($2, 2, length($2) - 3) ".s"; next }
    f != "" && NF { sub(/[ \t]*\/\/.*$/, ""); sub(/^[ \t]+/, ""); print > f }'
(cd "$tmp/k" && for s in *.s; do echo "${s%.s} $(sha256sum < "$s" | cut -d' ' -f1)"; done) | LC_ALL=C sort
if [ -n "${DUMP:-}" ]; then mkdir -p "$DUMP"; cp "$tmp"/k/*.s "$DUMP"/; fi
