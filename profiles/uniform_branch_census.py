#!/usr/bin/env python3
"""Census of wave-uniform decisions that go through lane masks, per kernel of a device-assembly listing.

    python3 profiles/uniform_branch_census.py <listing.s> [--kernel SUBSTRING] [--list] [--json]

Reads a listing as profiles/device_asm.sh writes it (fast.s, ...) or a disassembly of the code object (llvm-objdump -d); runs on a CPU.  A decision that is the same for every lane of a
wave can be taken on the scalar condition code (s_cmp; s_cbranch_scc).  The compiler's long forms, counted here per kernel:

  cselect    s_cselect_b64 <pair>, -1, 0            a scalar condition turned into a lane mask
  vcc_branch s_cbranch_vccz / s_cbranch_vccnz whose vcc was written by s_and_b64 / s_andn2_b64 vcc, exec, <pair>
             (a uniform branch on such a mask; the last write of vcc in front of the branch decides, across labels too)
  scalar_cmp v_cmp_* whose sources are all scalar registers or constants (a compare of uniform values on the vector unit)

and, for scale, all s_cbranch_vcc* and all s_cbranch_scc* of the kernel.  --list prints every counted instruction with its line in
the listing and, where the listing was compiled with debug info (.loc directives), its source line.  Counts are static: how often a
wave passes an instruction is read off the listing along the wave's path, not here.
"""
import argparse
import json
import re
import sys

KERNEL = re.compile(r'^(?:[0-9a-f]+ <)?(_Z\w+|[A-Za-z_]\w*)>?:\s*(;.*)?$')
VREG = re.compile(r'\bv(\d+|\[\d+:\d+\])')
CSELECT = re.compile(r'^s_cselect_b64\s+\S+,\s*-1,\s*0$')
VCC_AND = re.compile(r'^s_andn?2?_b64\s+vcc,\s*exec,\s*\S+$')
WRITES_VCC = re.compile(r'^(?:[sv]_\w+\s+vcc\b|v_cmp\w*_e32\b|v_(?:addc?|subb?(?:rev)?)_co_u32_e32\b|v_div_scale_\w+\s+\S+,\s*vcc\b)')


def census(path):
    """{kernel: {'cselect': [...], 'vcc_branch': [...], 'scalar_cmp': [...], 'all_vcc_branches': n, 'all_scc_branches': n,
    'instructions': n}}; the lists hold (listing line, source 'file:line' or None, text)."""
    out = {}
    cur = None
    files = {}
    loc = None
    vcc_from_mask = False
    for no, raw in enumerate(open(path), 1):
        line = raw.split(';')[0].split('//')[0].rstrip()
        s = line.strip()
        if not s:
            continue
        m = KERNEL.match(line)
        if m and not line.startswith(('\t', ' ', '.')):
            name = m.group(1)
            cur = out.setdefault(name, {'cselect': [], 'vcc_branch': [], 'scalar_cmp': [], 'all_vcc_branches': 0, 'all_scc_branches': 0, 'instructions': 0})
            loc = None
            vcc_from_mask = False
            continue
        if s.startswith('.file'):
            f = re.match(r'\.file\s+(\d+)\s+(?:"([^"]*)"\s+)?"([^"]*)"', s)
            if f:
                files[f.group(1)] = f.group(3)
            continue
        if s.startswith('.loc'):
            f = s.split()
            if len(f) >= 3:
                loc = '%s:%s' % (files.get(f[1], f[1]).split('/')[-1], f[2])
            continue
        if s.startswith('.Lfunc_end'):
            cur = None
            continue
        if cur is None or s.startswith('.') or s.endswith(':'):
            continue
        cur['instructions'] += 1
        rec = (no, loc, s)
        if CSELECT.match(s):
            cur['cselect'].append(rec)
        if s.startswith('s_cbranch_vcc'):
            cur['all_vcc_branches'] += 1
            if vcc_from_mask:
                cur['vcc_branch'].append(rec)
        elif s.startswith('s_cbranch_scc'):
            cur['all_scc_branches'] += 1
        if s.startswith('v_cmp') and not s.startswith('v_cmpx'):
            ops = s.split(None, 1)[1] if ' ' in s else ''
            srcs = ops.split(',')[0 if s.split()[0].endswith('_e32') else 1:]
            if srcs and not any(VREG.search(o) for o in srcs):
                cur['scalar_cmp'].append(rec)
        if VCC_AND.match(s):
            vcc_from_mask = True
        elif WRITES_VCC.match(s):
            vcc_from_mask = False
    return {k: v for k, v in out.items() if v['instructions']}


def counts(c):
    return {k: (len(v) if isinstance(v, list) else v) for k, v in c.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('listing')
    ap.add_argument('--kernel', default='', help='only kernels whose (mangled) name contains this')
    ap.add_argument('--list', action='store_true', help='every counted instruction')
    ap.add_argument('--json', action='store_true')
    a = ap.parse_args()
    res = {k: v for k, v in census(a.listing).items() if a.kernel in k}
    if a.json:
        json.dump({k: counts(v) for k, v in res.items()}, sys.stdout, indent=1)
        print()
        return
    for k, v in res.items():
        c = counts(v)
        print('%s\n  instructions %d  cselect %d  vcc_branch %d (of %d s_cbranch_vcc*)  scalar_cmp %d  s_cbranch_scc* %d' % (
            k, c['instructions'], c['cselect'], c['vcc_branch'], c['all_vcc_branches'], c['scalar_cmp'], c['all_scc_branches']))
        if a.list:
            for key in ('cselect', 'vcc_branch', 'scalar_cmp'):
                for no, loc, s in v[key]:
                    print('    %-10s %6d  %-28s %s' % (key, no, loc or '-', s))


if __name__ == '__main__':
    main()
