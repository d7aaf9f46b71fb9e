#!/usr/bin/env python3
"""Do two builds of the library hold the same device code?  (CPU; no GPU needed.)  For every gfx950 code object of each library
(tools/code_objects.py) the `llvm-objdump -d` text is cut into kernels; the two sets of kernel names must be equal and every kernel's
instructions identical (addresses and encodings are left out, so a kernel that merely moved inside its code object compares equal).  Also says
whether the code objects are byte-equal.  Exit code 0 = no difference.
usage: python tools/kernel_diff.py A.so B.so"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from code_objects import OBJDUMP, code_objects  # noqa: E402


def kernels(path):
    """({kernel name: [instruction text]}, [sha256 of each code object])"""
    out, shas = {}, []
    for co in code_objects(path):
        shas.append(hashlib.sha256(co).hexdigest())
        with tempfile.NamedTemporaryFile(suffix='.co', delete=False) as f:
            f.write(co)
            name = f.name
        try:
            txt = subprocess.run([OBJDUMP, '-d', '--no-show-raw-insn', '--no-leading-addr', name], capture_output=True, text=True, check=True).stdout
        finally:
            os.unlink(name)
        cur = None
        for line in txt.splitlines():
            m = re.match(r'^(?:[0-9a-f]+ )?<(\S+)>:$', line)
            if m:
                assert m.group(1) not in out, m.group(1)
                cur = out[m.group(1)] = []
            elif cur is not None and line.strip():
                cur.append(re.sub(r'\s*//.*$', '', line).strip())   # the trailing comment holds the address and the encoding
    return out, shas


def main():
    a, b = sys.argv[1:3]
    (ka, sa), (kb, sb) = kernels(a), kernels(b)
    only = sorted(set(ka) ^ set(kb))
    differ = sorted(n for n in set(ka) & set(kb) if ka[n] != kb[n])
    print(f'{a}: {len(sa)} code objects, {len(ka)} kernels, {sum(map(len, ka.values()))} instructions')
    print(f'{b}: {len(sb)} code objects, {len(kb)} kernels, {sum(map(len, kb.values()))} instructions')
    print(f'kernel names in one library only: {len(only)}' + ''.join(f'\n    {n}' for n in only))
    print(f'kernels compared: {len(set(ka) & set(kb))}; with different instructions: {len(differ)}' + ''.join(f'\n    {n}' for n in differ))
    print(f'code objects byte-equal: {sum(x == y for x, y in zip(sa, sb))} of {len(sa)}' if len(sa) == len(sb) else 'code objects: counts differ')
    sys.exit(1 if only or differ else 0)


if __name__ == '__main__':
    main()
