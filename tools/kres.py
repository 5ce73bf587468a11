#!/usr/bin/env python3
"""tools/kres.py K [FILTER] [EXTRA FLAGS...] -- per-kernel resource use (VGPRs, scratch, SGPR / VGPR
spills, occupancy) of the fast march object for depth lanes K, from the compiler's
-Rpass-analysis=kernel-resource-usage remarks; FILTER: a substring of the demangled template
arguments (e.g. "4, 2, true").

tools/kres.py --src FILE [--csrc DIR] [FILTER] [EXTRA FLAGS...] -- the same for every kernel of
another source file of csrc/ (e.g. vr_project.hip; no K), with each kernel's code length in bytes
(the size of its symbol in the device object); DIR: another checkout's csrc directory."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin/"
argv = sys.argv[1:]
src, csrc = "vr_march.hip", __file__.rsplit("/tools/", 1)[0] + "/volume_renderer_amd/csrc"
while argv and argv[0] in ("--src", "--csrc"):
    if argv[0] == "--src":
        src = argv[1]
    else:
        csrc = argv[1]
    argv = argv[2:]
march = src == "vr_march.hip"
K = argv.pop(0) if march else None
flt = argv[0] if argv else ""
extra = argv[1:]
obj = "/dev/null" if march else tempfile.mkstemp(suffix=".co")[1]
cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
       "-fno-slp-vectorize"] + (["-DVR_MARCH_FAST=1", f"-DVR_MARCH_K={K}"] if march else []) + \
      ["--offload-device-only"] + ([] if march else ["--no-gpu-bundle-output"]) + \
      ["-c", src, "-o", obj, "-Rpass-analysis=kernel-resource-usage"] + extra
out = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True).stderr
size, demangled = {}, {}
if not march:  # the function symbols of the device object: size, and the demangled name (-C, same order)
    def symtab(*opt):
        t = subprocess.run([LLVM + "llvm-objdump", "-t", *opt, obj], capture_output=True, text=True).stdout
        return re.findall(r"^[0-9a-f]{16} \S+\s+F \.text\s+([0-9a-f]+) (?:\.\w+ )?(.*)$", t, re.M)
    for (n, name), (_, dname) in zip(symtab(), symtab("-C")):
        size[name] = int(n, 16)
        demangled[name] = dname
    os.unlink(obj)
cur, rows = None, []
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        if march:
            mg = re.search(r"march_kernelI(.*?)EEv", m.group(1))
            args = re.findall(r"L([ib])(\d+)E", mg.group(1)) if mg else []
            dm = "march_kernel<" + ", ".join(v if t == "i" else ("true" if v == "1" else "false") for t, v in args) + \
                ">" if mg else m.group(1)
        else:  # the kernel's name and template arguments, without its parameter list
            dm = re.sub(r"^(void )?(vr::)?|\(.*$", "", demangled.get(m.group(1), m.group(1)))
        cur = {"name": dm, "code": size.get(m.group(1))}
        rows.append(cur)
        continue
    m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]*\])?):\s+(\S+)", line)
    if m and cur is not None:
        cur[m.group(1).strip()] = m.group(2)
for r in rows if march else sorted(rows, key=lambda r: r["name"]):
    if march and "march_kernel" in r["name"] and flt in r["name"]:
        args = r["name"].split("march_kernel<", 1)[1].split(">")[0]
        print(f"<{args}>  vgpr {r.get('VGPRs')}  scratch {r.get('ScratchSize [bytes/lane]')}  sgpr_spill "
              f"{r.get('SGPRs Spill')}  vgpr_spill {r.get('VGPRs Spill')}  occ {r.get('Occupancy [waves/SIMD]')}")
    elif not march and flt in r["name"]:
        print(f"{r['name']}  vgpr {r.get('VGPRs')}  sgpr {r.get('TotalSGPRs')}  scratch {r.get('ScratchSize [bytes/lane]')}  "
              f"occ {r.get('Occupancy [waves/SIMD]')}  code {r['code']}")
if not rows:
    sys.exit(out)
