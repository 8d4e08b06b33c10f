#!/usr/bin/env python3
"""Per kernel of device assembly files (hipcc ... -cuid=compare --offload-device-only -S): allocated VGPRs and SGPRs, scratch and LDS bytes,
instructions, FP64 VALU instructions (v_*_f64), and the waves per SIMD the VGPRs admit on gfx950 (512 per SIMD lane, allocated in
blocks of 8, at most 8 waves).
  python3 profiles/asm_figures.py A/rt_hits.s [B/rt_hits.s]     -> one line per kernel; with two files, both figures side by side"""
import re
import sys


def figures(path):
    out, name, body = {}, None, []
    text = open(path).read()
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and name is None and ".amdhsa_kernel " + m.group(1) in text:
            name, body = m.group(1), []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                ins = [l.split()[0] for l in body if re.match(r"^\s+[a-z]\w+", l) and not l.lstrip().startswith((".", ";"))]
                out[name] = {"instructions": len(ins), "fp64": sum(1 for i in ins if i.startswith("v_") and "f64" in i)}
                name = None
            else:
                body.append(line)
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        f = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
        k = out[m.group(1)]
        k["lds"], k["scratch"] = int(f["group_segment_fixed_size"]), int(f["private_segment_fixed_size"])
    for m in re.finditer(r"- \.agpr_count:.*?\.name:\s+(\S+).*?\.sgpr_count:\s+(\d+).*?\.vgpr_count:\s+(\d+)", text, re.S):
        k = out[m.group(1)]
        k["sgpr"], k["vgpr"] = int(m.group(2)), int(m.group(3))
        k["waves"] = min(8, 512 // (-(-k["vgpr"] // 8) * 8))
    return out


KEYS = ("vgpr", "sgpr", "scratch", "lds", "instructions", "fp64", "waves")
files = [figures(p) for p in sys.argv[1:3]]
print("kernel  " + "  ".join(KEYS))
for name in files[0]:
    short = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", name)
    short = re.match(r"[a-z_]+", short).group(0) if short != name else name
    cols = ["/".join(str(f[name][k]) for f in files if name in f) for k in KEYS]
    print(short + "  " + "  ".join(cols))
print("file  instructions " + "/".join(str(sum(k["instructions"] for k in f.values())) for f in files)
      + "  fp64 " + "/".join(str(sum(k["fp64"] for k in f.values())) for f in files))
