#!/usr/bin/env python3
"""tools/isa_hot.py [ASM] [--all] [--dump] [--classes] [--waves N] -- the lit wave-iteration of the
production march kernel's sample loop (/tmp/probe.s from tools/isa_probe.sh), counted and weighted.

The loop is the tame (finite, NANCHK = false) copy of the depth-lane sample loop whose box is whole:
among the depth-2 loops that hold the depth-lane compositing (a DPP quad_perm instruction), the one
with the fewest NaN tests, and of those the first.  All of its blocks count -- one lit iteration runs
through the whole loop -- minus those of the global-memory fall-backs (64-bit addressing:
v_lshl_add_u64 / v_mad_u64_u32) and of NaN-checking code (v_cmp_o_f32 / v_cmp_u_f32), which this loop
of the production build does not have (--all keeps them).

Every VALU instruction is weighted by its measured issue cost, cycles per wave-instruction per SIMD
at the nominal clock from tools/microbench/valu_costs.json (written by tools/microbench/valu_rates
on the GPU; --waves picks the occupancy it was measured at, default 5, the march kernel's).  An
instruction that was not measured takes the cost of its class: the plain 32-bit ops that of
v_add_f32, everything else that of v_med3_f32 (the slow class), transcendentals that of v_rsq_f32.
A static estimate, for comparing builds and for the issue-time model of DESIGN.md s5."""
import collections
import json
import os
import re
import sys

argv = sys.argv[1:]
waves = "5"
if "--waves" in argv:
    i = argv.index("--waves")
    waves = argv[i + 1]
    del argv[i:i + 2]
paths = [a for a in argv if not a.startswith("--")]
path = paths[0] if paths else "/tmp/probe.s"
s = open(path).read()
name = re.search(r"(_ZN2vr4fast12march_kernelILi2ELi1ELb1ELb0ELb1ELb0ELi(?:1664|2040)ELi0E(?:Li\d+E)?EEvNS_12RenderParamsE):", s).group(1)
body = s[s.index(name + ":"):s.index(".Lfunc_end", s.index(name + ":"))].split("\n")
blocks, cur = [], None
for l in body:
    m = re.match(r"^(\.LBB\d+_\d+):(.*)", l) or re.match(r"^; %bb\.(\d+):(.*)", l)
    if m:
        cur = {"name": m.group(1), "hdr": m.group(2), "ins": []}
        blocks.append(cur)
        continue
    t = l.strip()
    if cur is None or not t or t.startswith((".", ";")):
        continue
    cur["ins"].append(t.split(";")[0].strip())
# the depth-2 loops that composite a depth-lane group: headers named in the block comments
# ('in Loop: Header=BBx_y Depth=2'), in order of appearance
group = [i for i, b in enumerate(blocks) if any("quad_perm:[0,0,2,2]" in x for x in b["ins"])]
hdrs = []
for i in group:
    m = re.search(r"Header=BB(\d+_\d+) Depth=2", blocks[i]["hdr"])
    if m and m.group(1) not in hdrs:
        hdrs.append(m.group(1))
NAN = ("v_cmp_o_f32", "v_cmp_u_f32")
BIG = ("v_lshl_add_u64", "v_mad_u64_u32")
best = None
for h in hdrs:
    lp = [b for b in blocks if f"Header=BB{h} " in b["hdr"] or b["name"] == f".LBB{h}"]
    nan = sum(1 for b in lp for x in b["ins"] if x.startswith(NAN))
    if best is None or nan < best[1]:
        best = (h, nan, lp)
hdr, _, loop = best
hot = loop if "--all" in argv else [b for b in loop if not any(x.startswith(NAN + BIG) for x in b["ins"])]


def mnemonic(x):
    """v_fmac_f32_dpp for a VOP2 with a DPP operand; the _e32 / _e64 encoding suffix dropped except
    where the two were measured apart (v_cndmask_b32)."""
    op = x.split()[0]
    if ("quad_perm" in x or "row_" in x) and not op.endswith("_dpp"):
        op += "_dpp"
    base = re.sub(r"_e(32|64)$", "", op)
    return op if base == "v_cndmask_b32" else base


tab_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "microbench", "valu_costs.json")
costs = json.load(open(tab_path))["waves_" + waves]["wall"] if os.path.exists(tab_path) else {}
FAST = ("v_add_", "v_sub", "v_mul_f32", "v_fma", "v_mac", "v_and_b32", "v_or_b32", "v_xor_b32", "v_not_b32", "v_mov_b32")
TRANS = ("v_rsq", "v_sqrt", "v_exp", "v_rcp", "v_log", "v_sin", "v_cos")


def cost(op):
    if op == "v_cndmask_b32_e32":
        # after the v_cmp that sets vcc, as the compiler emits it: the measured pair less the compare
        # (alone, with a vcc that no VALU instruction of the loop wrote, it measured 23 cycles)
        return costs.get("v_cmp+v_cndmask", 0) - costs.get("v_cmp_gt_f32", 0)
    if op in costs:
        return costs[op]
    if op.startswith("v_cmp"):
        return costs.get("v_cmp_gt_f32", 0)
    if op.endswith("_dpp"):
        return costs.get("v_fmac_f32_dpp" if op != "v_mov_b32_dpp" else op, 0)
    if op.startswith(TRANS):
        return costs.get("v_rsq_f32", 0)
    if op.startswith(FAST) and "add3" not in op and "lshl" not in op and "u64" not in op:
        return costs.get("v_add_f32", 0)
    return costs.get("v_med3_f32", 0)


c = collections.Counter(mnemonic(x) for b in hot for x in b["ins"])
valu = {k: n for k, n in c.items() if k.startswith("v_")}
nvalu = sum(valu.values())
trans = sum(n for k, n in valu.items() if k.startswith(TRANS))
plain = costs.get("v_add_f32", 0)
slow = sum(n for k, n in valu.items() if not k.startswith(TRANS) and cost(k) > 1.3 * plain) if costs else 0
cycles = sum(n * cost(k) for k, n in valu.items())
lds = sum(n for k, n in c.items() if k.startswith("ds_"))
vmem = sum(n for k, n in c.items() if k.startswith(("global_", "buffer_", "flat_", "scratch_")))
salu = sum(n for k, n in c.items() if k.startswith("s_"))
print(f"loop BB{hdr}: {len(loop)} blocks, counted {len(hot)}: instructions {sum(c.values())}, VALU {nvalu} "
      f"(slow class {slow}, transcendental {trans}), SALU {salu}, LDS {lds}, VMEM {vmem}, v_mov_b32 {c['v_mov_b32']}, "
      f"DPP {sum(n for k, n in c.items() if k.endswith('_dpp'))}, v_rndne {c['v_rndne_f32']}, s_nop {c['s_nop']}; "
      f"weighted VALU issue {cycles:.0f} nominal cycles per lit iteration ({waves} waves per SIMD)")
if "--classes" in argv:
    for k, n in sorted(valu.items(), key=lambda kv: -kv[1] * cost(kv[0])):
        print(f"  {k:24s} {n:4d} x {cost(k):5.2f} = {n * cost(k):7.1f}{'' if k in costs else '  (class cost)'}")
if "--dump" in argv:
    for b in hot:
        print(b["name"], b["hdr"][:80])
        for x in b["ins"]:
            print("   ", x)
