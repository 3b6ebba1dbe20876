#!/usr/bin/env python3
"""Compare the kernels of two device assembly files (``hipcc --cuda-device-only -S``, as build.py writes
``build/C/gemv.s``): the same kernel symbols, and for each the same text from its label to ``.end_amdhsa_kernel``.
The order of the kernels in the file may differ (a host-side refactor moves the instantiation order); the function
index in block labels (``.LBB<index>_<block>``) follows that order and is masked. Exit 1 on any difference.

Usage: ``python tools/asm_kernels_diff.py OLD.s NEW.s``"""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M):
        name = m.group(1)
        start = text.index(f"\n{name}:", 0) + 1
        end = text.index(".end_amdhsa_kernel", m.end())
        assert start < m.start() and name not in out, name
        body = re.sub(r"\bL?BB\d+_", "BB_", text[start:end])  # (labels, and the loop comments that name them)
        # (a label's loop comment is padded to a column: the padding changes with the digits of the masked index)
        out[name] = re.sub(r"(?m)^(\.BB_\d+:)[ \t]+;", r"\1 ;", body)
    return out


def main(old, new):
    a, b = kernels(old), kernels(new)
    only = sorted(set(a) ^ set(b))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    for n in only:
        print(("only in old: " if n in a else "only in new: ") + n)
    for n in differ:
        print("text differs: " + n)
    print(f"{len(a)} / {len(b)} kernel symbols, {len(only)} unmatched, {len(differ)} with different text")
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
