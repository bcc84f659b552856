#!/usr/bin/env python3
"""Price the VALU blocks of the fp32 inference kernel from its assembly (hipcc -S --offload-device-only of csrc/sn_mlp_fwd_f32g.hip with
-DSN_F32G_AB: one instantiation): the non-MFMA VALU instructions of the unit loop, gap by gap (a gap = the instructions between two MFMAs),
and their cost by the measured law of DESIGN.md 3.1 -- a gap with n VALU instructions costs 9.6 + 4 n cycles of matrix time.
A gap that holds a wave-uniform branch lists every side of it, in text order: the sum is an upper bound for such a gap.
usage: f32g_valu_gaps.py kernel.s [min_n]      (gaps with at least min_n VALU instructions are listed, default 12)"""
import re
import sys

path = sys.argv[1]
min_n = int(sys.argv[2]) if len(sys.argv) > 2 else 12
lines = open(path).read().split("\n")
# everything behind the kernel's one barrier: the unit loop (hipcc lays the end of the loop body out in front of the loop header) and the
# few dozen one-time instructions of the prologue, which land in the first gap
start = max(i for i, l in enumerate(lines) if l.strip().startswith("s_barrier"))
gaps, n, names = [], 0, []
for l in lines[start:]:
    t = l.strip().split(";")[0].strip()
    if not t or t.startswith(".") or t.endswith(":"):
        continue
    op = t.split()[0]
    if op == "s_endpgm":
        break
    if op.startswith("v_mfma"):
        gaps.append((n, names)); n, names = 0, []
    elif op.startswith("v_"):
        n += 1; names.append(op)
gaps.append((n, names))
total = sum(g[0] for g in gaps)
used = [g for g in gaps if g[0] > 0]
cyc = sum(9.6 + 4 * g[0] for g in used)
mfma = len(gaps) - 1
print("%s: %d MFMAs, %d non-MFMA VALU instructions in %d gaps: %.0f cycles = %.2f %% of %d x 64" % (path, mfma, total, len(used), cyc,
                                                                                             100 * cyc / (64.0 * mfma), mfma))
for i, (k, nm) in enumerate(gaps):
    if k >= min_n:
        print("  gap before MFMA %5d: %4d VALU = %5.0f cycles" % (i, k, 9.6 + 4 * k))
