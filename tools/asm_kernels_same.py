#!/usr/bin/env python3
"""Are some kernels of two builds the same gfx950 code?  For every kernel whose mangled name matches one of the given regular
expressions: its instructions and .amdhsa_kernel descriptor are cut out of both assembly files (`hipcc -O3 --offload-arch=gfx950
--save-temps` leaves `<source>-hip-amdgcn-amd-amdhsa-gfx950.s`), comments are stripped, the file-wide function ordinal in local labels
(.LBB<n>_k) is replaced by N, and the two texts are compared.  Needs no GPU.

    python tools/asm_kernels_same.py PARENT.s THIS.s 'k_reduce_allENS' 'k_reduce_all_sgdENS' 'k_gather_rowsI'

--rename OLD=NEW (mangled names, repeatable): kernel OLD of the first file is kernel NEW of the second.  Such a pair is not expected to be
the same text (its arguments moved); it is listed instead: instruction count, VGPRs, SGPRs, LDS, scratch and kernarg bytes of both, whether
the kernel's floating-point vector instructions are the same sequence of mnemonics in program order (register names, and so the order of
the two halves of a packed pair, do not count; a half moved across a branch does, and is shown), and which mnemonics the code gained or
lost.  It breaks a resource condition when it has scratch, more VGPRs or another LDS size than OLD.
"""
import collections
import difflib
import re
import sys

FIELDS = (("VGPRs", "next_free_vgpr"), ("SGPRs", "next_free_sgpr"), ("LDS", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size"),
          ("kernarg", "kernarg_size"))


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


def mnemonics(lines):
    """the instructions' mnemonics, in order (no labels, no directives)"""
    return [m.group(1) for m in (re.match(r"\s+([a-z]\w*)", ln) for ln in lines) if m]


def descriptor(lines):
    found = dict(m.groups() for m in (re.match(r"\s+\.amdhsa_(\w+)\s+(\S+)", ln) for ln in lines) if m)
    return {label: int(found[key]) for label, key in FIELDS}


def fp_vector(ops):
    """the floating-point vector instructions, in program order"""
    return [op for op in ops if re.match(r"v_\w+_f(16|32|64)(_e32|_e64|_dpp|_sdwa)?$", op)]


def renamed(a, b, old, new):
    x, y = cut(a, old), cut(b, new)
    ox, oy, dx, dy = mnemonics(x), mnemonics(y), descriptor(x), descriptor(y)
    fx, fy = fp_vector(ox), fp_vector(oy)
    gained, lost = collections.Counter(), collections.Counter()
    for tag, i0, i1, j0, j1 in difflib.SequenceMatcher(None, ox, oy, autojunk=False).get_opcodes():
        if tag != "equal":
            lost.update(ox[i0:i1])
            gained.update(oy[j0:j1])
    moved = gained & lost                    # the same mnemonic at another place: scheduling
    gained, lost = gained - moved, lost - moved
    bad = [why for why, cond in (("scratch", dy["scratch"] != 0), ("more VGPRs", dy["VGPRs"] > dx["VGPRs"]), ("LDS differs", dy["LDS"] != dx["LDS"])) if cond]
    print(f"{old}\n -> {new}")
    print(f"    instructions {len(ox)} -> {len(oy)}; " + "; ".join(f"{k} {dx[k]} -> {dy[k]}" for k, _ in FIELDS))
    print(f"    floating-point vector instructions: {len(fx)} against {len(fy)}: {'the SAME sequence' if fx == fy else 'ANOTHER sequence'}")
    if fx != fy:
        print("\n".join("      " + ln for ln in list(difflib.unified_diff(fx, fy, lineterm="", n=2))[2:]))
    fmt = lambda c: ", ".join(f"{op} x{k}" for op, k in sorted(c.items())) or "none"
    print(f"    all instructions, by mnemonic: gained {fmt(gained)}; lost {fmt(lost)}; at another place {fmt(moved)}")
    print(f"    resources: {'OK' if not bad else 'NOT OK: ' + ', '.join(bad)}")
    return bool(bad), fx != fy


def main():
    args, renames = [], []
    it = iter(sys.argv[1:])
    for arg in it:
        if arg == "--rename":
            renames.append(tuple(next(it).split("=", 1)))
        else:
            args.append(arg)
    if len(args) < 3:
        sys.exit(__doc__)
    a, b = open(args[0]).read(), open(args[1]).read()
    pattern = "|".join(f"(?:{p})" for p in args[2:])
    olds = {old for old, _ in renames}
    names = sorted(n for n in set(re.findall(r"^(\w+):", a, flags=re.M)) if re.search(pattern, n) and ".amdhsa_kernel " + n in a and n not in olds)
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
    if renames:
        print()
        verdicts = [renamed(a, b, old, new) for old, new in renames]
        wrong, other_fp = sum(v[0] for v in verdicts), sum(v[1] for v in verdicts)
        print(f"\n{len(renames)} renamed kernels listed: {wrong} break a resource condition, {other_fp} have another floating-point sequence.")
        differ += wrong + other_fp
    return 1 if differ or not (names or renames) else 0


if __name__ == "__main__":
    sys.exit(main())
