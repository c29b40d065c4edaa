#!/usr/bin/env python3
"""Are the kernels of two hipcc -S --cuda-device-only listings the same code?  isa_diff.py a.s b.s
Per kernel the text from its label to .end_amdhsa_kernel (the .amdhsa_* block included), without comment-only lines, trailing comments and
debug-line directives, .LBB labels renumbered by order of appearance.  Prints one line per kernel (instructions, VGPR, SGPR, LDS, scratch of
both sides where they differ) and exits 1 when any kernel differs or exists on one side only."""
import re, sys


def clean(text):
    names, lines = {}, []
    for l in text.splitlines():
        l = re.sub(r'\s*;.*$', '', l).rstrip()
        if not l.strip() or re.match(r'\s*\.(loc|file|cfi_|p2align)', l):
            continue
        lines.append(re.sub(r'\.L(BB|tmp|func_\w+?)\d+(_\d+)?', lambda g: names.setdefault(g.group(0), f".L{g.group(1)}#{len(names)}"), l))
    return lines


def kernels(path):
    """name -> (cleaned lines, figures); device functions kept out of line are listed too, from their label to .Lfunc_end"""
    s = open(path).read()
    out = {}
    kernel_names = set(re.findall(r'^\s*\.amdhsa_kernel (\S+)', s, re.M))
    for name in re.findall(r'^\s*\.type\s+(_Z\w+),@function', s, re.M):
        end = r'^\s*\.end_amdhsa_kernel' if name in kernel_names else r'^\.Lfunc_end\d+:'
        m = re.search(r'^' + re.escape(name) + r':[^\n]*\n(.*?' + end + ')', s, re.S | re.M)
        raw, lines = m.group(1), clean(m.group(1))
        f = {"insts": 0}
        for l in lines:
            if l.strip().startswith('.section'):
                break
            f["insts"] += not l.strip().startswith('.') and not l.endswith(':')
        for key, tag in (("next_free_vgpr", "vgpr"), ("next_free_sgpr", "sgpr"), ("group_segment_fixed_size", "lds"), ("private_segment_fixed_size", "scratch")):
            g = re.search(r'\.amdhsa_' + key + r'\s+(\d+)', raw)
            if g:
                f[tag] = int(g.group(1))
        out[name] = (lines, f)
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
differ = 0
for k in sorted(set(a) | set(b)):
    if k not in a or k not in b:
        print(f"ONLY {'a' if k in a else 'b'}  {k}")
        differ += 1
    elif a[k][0] == b[k][0]:
        print(f"same    {k}  {a[k][1]}")
    else:
        print(f"DIFFER  {k}\n   a: {a[k][1]}\n   b: {b[k][1]}")
        differ += 1
sys.exit(1 if differ else 0)
