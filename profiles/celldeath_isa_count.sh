#!/bin/bash
# FP64 VALU instructions of each kernel of csrc/k_celldeath.hip, by mnemonic, from the ISA at the Makefile's flags
# (DESIGN.md 4i).  Static counts: both models' and the limits' branches are counted, not all are taken.
# Usage: profiles/celldeath_isa_count.sh   (writes nothing; prints "kernel mnemonic count" and a total per kernel)
set -e
cd "$(dirname "$0")/../cardiac-ablation-ecm2_amd"
${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics --cuda-device-only -S \
   csrc/k_celldeath.hip -o - |
awk '/^_ZN4ecm2[A-Za-z0-9_]*k_celldeath[A-Za-z0-9_]*:/ { name = $1; sub(/^_ZN4ecm212_GLOBAL__N_1[0-9]+/, "", name); sub(/E[A-Za-z0-9_]*:$/, "", name) }
     /^[ \t]+v_[a-z0-9_]*f64/ { m = $1; sub(/_e(32|64)$/, "", m); c[name " " m]++; t[name]++ }
     END { for (k in c) print k, c[k]; for (k in t) print k, "total", t[k] }' | sort
