#!/usr/bin/env python3
"""Are some kernels of two builds the same gfx950 code?  For every kernel whose mangled name matches one of the given regular
expressions: its instructions and .amdhsa_kernel descriptor are cut out of both assembly files (`hipcc -O3 --offload-arch=gfx950
--save-temps` leaves `<source>-hip-amdgcn-amd-amdhsa-gfx950.s`), comments are stripped, the file-wide function ordinal in local labels
(.LBB<n>_k) is replaced by N, and the two texts are compared.  Needs no GPU.

    python tools/asm_kernels_same.py PARENT.s THIS.s 'k_reduce_allENS' 'k_reduce_all_sgdENS' 'k_gather_rowsI'
"""
import difflib
import re
import sys


def cut(text, name):
    body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\s*\.size\s+" + re.escape(name) + r",", text, flags=re.M | re.S).group(1)
    assert ".amdhsa_kernel " + name in body and ".end_amdhsa_kernel" in body      # the descriptor lies between the label and .size
    out = []
    for line in body.splitlines():
        line = re.sub(r";.*$", "", line).rstrip()
        line = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1N", line)
        if line.strip():
            out.append(line)
    return out


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    a, b = open(sys.argv[1]).read(), open(sys.argv[2]).read()
    pattern = "|".join(f"(?:{p})" for p in sys.argv[3:])
    names = sorted(n for n in set(re.findall(r"^(_Z\w+):", a, flags=re.M)) if re.search(pattern, n) and ".amdhsa_kernel " + n in a)
    differ = 0
    for n in names:
        if n + ":" not in b:
            print(f"{n}: MISSING from the second file")
            differ += 1
            continue
        x, y = cut(a, n), cut(b, n)
        differ += x != y
        print(f"{n}: {len(x)} lines against {len(y)}: {'IDENTICAL' if x == y else 'DIFFERENT'}")
        if x != y:
            print("\n".join(list(difflib.unified_diff(x, y, lineterm=""))[:60]))
    print(f"\n{len(names)} kernels compared, {differ} differ.")
    return 1 if differ or not names else 0


if __name__ == "__main__":
    sys.exit(main())
