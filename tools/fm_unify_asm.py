#!/usr/bin/env python3
"""Device code of the canonical-FM / valued / field-aware kernels, this tree against another (no
GPU needed).  Compiles xf_fm_canonical.hip, xf_valued.hip and xf_ffm.hip (where OTHER has it) of
both trees for gfx950 with build.py's FLAGS, splits the assembly per kernel and pairs every
kernel of OTHER with its successor here: the kernel of the same name where there is one, else
(OTHER older than the VAL fold) k_fmc_*<...> with k_fmc_*<..., false>, k_val_fm_*<...> /
k_val_heavy_partial with k_fmc_*<..., true>.  Kernels only this tree has (the emitting
instantiations, OPT = 2) are listed after the pairs with their resources.  Per pair: instructions, the resources
(next_free_vgpr / next_free_sgpr / accum_offset / LDS / scratch), whether the multiset of
mnemonics is equal (s_load_*, s_waitcnt, s_nop, s_mov_* set aside: kernarg layout and SGPR
numbering) and whether the whole mnemonic sequence is.  Prints a markdown table; --diff shows the
sequence diff of the pairs that differ.
  python tools/fm_unify_asm.py OTHER_TREE [--diff]"""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xflow_amd import build  # noqa: E402

FILES = ("xf_fm_canonical.hip", "xf_valued.hip", "xf_ffm.hip")
RES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size",
       "private_segment_fixed_size")
ASIDE = re.compile(r"s_load_|s_waitcnt|s_nop|s_mov_")


def kernels(tree, tmp):
    """{demangled name without arguments: (mnemonics, resources)} of a tree's two files"""
    out = {}
    for f in FILES:
        if not os.path.exists(os.path.join(tree, "xflow_amd", "csrc", f)):
            continue
        flags = [x.replace(ROOT, tree) if x.startswith("-I") else x for x in build.FLAGS]
        asm = os.path.join(tmp, f + ".s")
        subprocess.check_call([build._hipcc()] + flags + ["-x", "hip", "--cuda-device-only", "-S",
                               os.path.join(tree, "xflow_amd", "csrc", f), "-o", asm],
                              stderr=subprocess.DEVNULL)
        text = open(asm).read()
        for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
            sym, block = m.group(1), m.group(2)
            res = tuple(int(re.search(r"\.amdhsa_%s (\d+)" % r, block).group(1)) for r in RES)
            body = text[text.index("\n%s:" % sym):]
            body = body[:body.index(".Lfunc_end")]
            ins = [l.split()[0] for l in (x.strip() for x in body.split("\n")[2:])
                   if l and l[0] not in ".;" and not l.split()[0].endswith(":")]
            name = subprocess.check_output(["c++filt", sym], text=True)
            name = name.strip().replace("(anonymous namespace)::", "")
            out[re.sub(r"\(.*", "", name).replace("void ", "")] = (ins, res)
    return out


def successor(name, new=()):
    if name in new or name.startswith("k_val_lr_") or name.startswith("k_fmc_heavy_finish"):
        return name
    val = "true" if name.startswith("k_val_") else "false"
    name = name.replace("k_val_fm_", "k_fmc_").replace("k_val_heavy_partial", "k_fmc_heavy_partial")
    return name[:-1] + ", %s>" % val if name.endswith(">") else name + "<%s>" % val


def main():
    other = os.path.abspath(sys.argv[1])
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        old, new = kernels(other, t1), kernels(ROOT, t2)
    print("| kernel of the other tree | kernel here | instructions | vgpr / sgpr / accum_offset / "
          "LDS / scratch | resources equal | multiset equal | sequence equal |")
    print("|---|---|---|---|---|---|---|")
    bad, seq_ne, diffs = 0, [], []
    for name in sorted(old):
        (i0, r0), (i1, r1) = old[name], new[successor(name, new)]
        core = [collections.Counter(x for x in i if not ASIDE.match(x)) for i in (i0, i1)]
        ok_r, ok_m, ok_s = r0 == r1 and r1[4] == 0, core[0] == core[1], i0 == i1
        bad += not (ok_r and ok_m)
        if not ok_s:
            seq_ne.append(name)
            diffs.append("\n".join(difflib.unified_diff(i0, i1, name, successor(name, new), lineterm="", n=2)))
        yn = lambda b: "yes" if b else "NO"  # noqa: E731
        n = str(len(i0)) if len(i0) == len(i1) else "%d -> %d" % (len(i0), len(i1))
        print("| `%s` | `%s` | %s | %s | %s | %s | %s |" % (
            name, successor(name, new), n, " / ".join(map(str, r1)), yn(ok_r), yn(ok_m), yn(ok_s)))
    fresh = sorted(set(new) - {successor(n, new) for n in old})
    if fresh:
        print("\n| kernel only here | instructions | vgpr / sgpr / accum_offset / LDS / scratch |")
        print("|---|---|---|")
        for name in fresh:
            ins, res = new[name]
            bad += res[4] != 0
            print("| `%s` | %d | %s |" % (name, len(ins), " / ".join(map(str, res))))
    print("\n%d kernels of the other tree, %d here; %d pairs differ in resources or multiset; "
          "%d differ in sequence" % (len(old), len(new), bad, len(seq_ne)))
    if "--diff" in sys.argv:
        print("\n".join(diffs))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
