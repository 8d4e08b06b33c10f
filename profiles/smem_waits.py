#!/usr/bin/env python3
"""How one kernel of a device assembly file (profiles/device_asm.sh: <build>.s) issues its scalar memory loads and waits for them.
A static reading of the instruction stream in program order, branches ignored - nothing is run:
  s_load            scalar memory loads (s_load_*) of the kernel
  waited within 3   those followed by an s_waitcnt with lgkmcnt(0) within the next three instructions: a load nothing is overlapped with
  waits ahead       s_waitcnt lgkmcnt(..) instructions from the kernel's first instruction up to the first, and up to the second,
                    v_rsq_f64 that follows the launch-table entry's load (the first s_load_dwordx4 whose base is not the kernarg
                    pointer s[0:1]).  In the one-wave trace kernels the first v_rsq_f64 is the ray generation's, the second the root
                    of the one-candidate wave's anchored test: the waits in front of it are what such a wave stands through before
                    its first useful result.
  python3 profiles/smem_waits.py A/fast.s '<0,0,0,0,1>'       the kernel: a substring of its mangled name, or rt_trace's template
                                                              arguments as <r,c,s,g,w> (REFRACT, COUNT, SS2, GRID, W1)"""
import re
import sys


def kernel_body(path, want):
    m = re.fullmatch(r"<([01]),([01]),([01]),([01]),([01])>", want)
    if m:
        want = "rt_traceI" + "".join("Lb%sE" % b for b in m.groups()) + "E"
    name, body = None, []
    for line in open(path):
        h = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if name is None:
            if h and want in h.group(1):
                name = h.group(1)
        elif line.startswith(".Lfunc_end"):
            break
        elif re.match(r"^\s+[a-z]\w+", line) and not line.lstrip().startswith((".", ";")):
            body.append(line.split(";")[0].strip())
    if name is None:
        sys.exit("no kernel matching %r in %s" % (want, path))
    return name, body


def is_lgkm_wait(ins):
    return ins.startswith("s_waitcnt") and "lgkmcnt" in ins


def figures(body):
    loads = [i for i, ins in enumerate(body) if ins.startswith("s_load_")]
    tight = sum(1 for i in loads if any(is_lgkm_wait(x) and "lgkmcnt(0)" in x for x in body[i + 1:i + 4]))
    entry = next((i for i in loads if body[i].startswith("s_load_dwordx4") and not re.search(r",\s*s\[0:1\]\s*,", body[i])), None)
    ahead = []
    if entry is not None:
        waits = 0
        for i, ins in enumerate(body):
            if is_lgkm_wait(ins):
                waits += 1
            elif i > entry and ins.startswith("v_rsq_f64"):
                ahead.append(waits)
                if len(ahead) == 2:
                    break
    return len(loads), tight, ahead


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    name, body = kernel_body(sys.argv[1], sys.argv[2])
    n, tight, ahead = figures(body)
    print("%s: s_load %d  waited within 3: %d  lgkmcnt waits ahead of the 1st / 2nd v_rsq_f64 after the entry load: %s"
          % (name, n, tight, " / ".join(str(a) for a in ahead) or "-"))
