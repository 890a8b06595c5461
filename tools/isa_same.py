#!/usr/bin/env python
"""Are two device listings of the engine the same code?  `isa_same.py a.s b.s` -> exit status 0 / 1.

The listings are what `hipcc <HIPCC_FLAGS without -fPIC -shared> -S --cuda-device-only` writes (the command of
tests/test_kernel_resources.py).  Host-only edits may reorder the instantiation of template kernels, and with it
the order of the functions and the function number in local labels; the source path changes the hash in the
__hip_cuid_ symbol.  So the text is compared symbol by symbol: the same set of symbols, the same body per symbol
(function number in .LBB<k>_<n>, .Lfunc_end<k> and their kin replaced, the __hip_cuid_ hash replaced), the same
.amdhsa_kernel .. .end_amdhsa_kernel block per kernel and the same metadata entry per kernel."""
import re
import sys

LABEL = re.compile(r'^([A-Za-z_$][\w$.]*):')
HEADER = ('\t.protected', '\t.globl', '\t.weak', '\t.hidden', '\t.p2align', '\t.type', '\t.section', '\t.text')
LOCAL = re.compile(r'\.L(BB|func_begin|func_end|JTI|tmp)\d+')
LOOP_NOTE = re.compile(r'\bBB\d+(?=_\d+ Depth)')   # the same number in the loop comments: "Header=BB71_2 Depth=1"
LABEL_PAD = re.compile(r'^(\.LBB#_\d+:)[ \t]+;', re.M)   # a label's comment column moves with the number's width
KERNEL = re.compile(r'^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel$', re.S | re.M)


def split(path):
    """-> ({symbol: body}, {kernel: descriptor block}, {kernel: metadata entry})"""
    text = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_', open(path).read())
    code, _, meta = text.partition('\t.amdgpu_metadata\n')
    code = LOOP_NOTE.sub('BB#', LOCAL.sub(lambda m: '.L' + m.group(1) + '#', code))
    lines = LABEL_PAD.sub(r'\1 ;', code).split('\n')
    starts = []
    for i, line in enumerate(lines):
        m = LABEL.match(line)
        if m:
            while i > 0 and lines[i - 1].startswith(HEADER):
                i -= 1
            starts.append((i, m.group(1)))
    bodies = {}
    for (a, name), (b, _) in zip(starts, starts[1:] + [(len(lines), None)]):
        if name in bodies:
            raise SystemExit('%s: symbol %s is defined twice' % (path, name))
        bodies[name] = '\n'.join(lines[a:b])
    bodies['<before the first symbol>'] = '\n'.join(lines[:starts[0][0]] if starts else lines)
    kernels = {m.group(1): m.group(0) for m in KERNEL.finditer(code)}
    entries = {}
    for entry in re.split(r'^(?=  - )', meta, flags=re.M)[1:]:
        name = re.search(r'^\s+\.name:\s+(\S+)', entry, re.M)
        if name:
            entries[name.group(1)] = entry
    return bodies, kernels, entries


def main(a, b):
    same = True
    for what, x, y in zip(('symbol', 'kernel descriptor', 'kernel metadata'), split(a), split(b)):
        for name in sorted(set(x) | set(y)):
            if name not in x or name not in y:
                print('%s %s: only in %s' % (what, name, b if name in y else a))
            elif x[name] != y[name]:
                print('%s %s: differs' % (what, name))
            else:
                continue
            same = False
        print('%d %s entries in %s, %d in %s' % (len(x), what, a, len(y), b))
    print('same device code' if same else 'DIFFERENT device code')
    return 0 if same else 1


if __name__ == '__main__':
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
