#!/bin/bash
# Per-kernel register / occupancy summary of a HIP source for gfx950, compiled device-only with the flags of
# csrc/Makefile (its CXXFLAGS with the default ARCH; EXTRA from the environment): scripts/regs.sh file.hip
f=${1:?usage: regs.sh file.hip}
root="$(cd "$(dirname "$0")/.." && pwd)"
mk="$root/rvc-maker_amd/csrc/Makefile"
hipcc=$(command -v hipcc || echo /opt/rocm/bin/hipcc)
arch=$(sed -n 's/^ARCH ?= //p' "$mk")
flags=$(sed -n 's/^CXXFLAGS := //p' "$mk")
flags=${flags//\$(ARCH)/$arch}
flags=${flags//\$(EXTRA)/$EXTRA}
tmp=$(mktemp -d)
# shellcheck disable=SC2086
"$hipcc" $flags --cuda-device-only -S "$f" -o "$tmp/regs.s" -Rpass-analysis=kernel-resource-usage 2>&1 |
  python3 -c '
import re, sys
rows, cur = [], None
for line in sys.stdin:
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = {"name": m.group(1)}; rows.append(cur); continue
    m = re.search(r"remark:\s+(VGPRs|AGPRs|VGPRs Spill|Occupancy \[waves/SIMD\]|ScratchSize \[bytes/lane\]): (\d+)", line)
    if m and cur is not None: cur[m.group(1).split()[0] + ("S" if "Spill" in m.group(1) else "")] = m.group(2)
for r in rows:
    print(r["name"][:80].ljust(80), "V", r.get("VGPRs"), "A", r.get("AGPRs"), "spill", r.get("VGPRsS"),
          "scratch", r.get("ScratchSize"), "occ", r.get("Occupancy"))'
rm -rf "$tmp"
