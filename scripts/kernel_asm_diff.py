#!/usr/bin/env python3
"""Are kernels of two builds the same instructions in the same order?  Compares gfx950 assembly listings of one source file
made at two commits:

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off --offload-device-only -S csrc/qcnn_glue.hip -o new.s
  (the same in a checkout of the other commit)                                                                   -o old.s
  kernel_asm_diff.py old.s new.s k_pack_u8_resized k_pack_u8_relaxed

Every function of old.s whose demangled-free name contains one of the given words is paired with the function of new.s that
contains the same word and has the same template VALUE arguments in front (Lb0 / Lb1: the mangled `false` / `true`); a kernel
may have gained template TYPE parameters, so names are not compared.  Of a body, comments, directives and local label NAMES
are dropped (labels are renumbered in order of appearance): what is compared is the instruction text, operands included.
Exit status 0: every pair identical."""
import re
import sys


def bodies(path):
    """{function name: [instruction lines]} of an assembly listing."""
    out, name, lines = {}, None, []
    for raw in open(path):
        line = raw.split(";", 1)[0].rstrip()
        m = re.match(r"^([A-Za-z_][\w.$]*):", line)
        if m and not m.group(1).startswith((".L", "BB")):
            name, lines = m.group(1), []
            out[name] = lines
            continue
        if name is None or not line.strip():
            continue
        s = line.strip()
        if s.startswith(".") and not s.startswith(".LBB"):
            if s.startswith((".Lfunc_end", ".section", ".end_amdhsa_kernel")):
                name = None
            continue
        lines.append(s)
    return out


def normalised(lines):
    labels = {}
    for s in lines:
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            labels.setdefault(m.group(1), "L%d" % len(labels))
    return [re.sub(r"\.LBB\w+", lambda m: labels.get(m.group(0), m.group(0)), s) for s in lines]


def key(name, word):
    """What identifies an instantiation across the two builds: the word and the bool template arguments."""
    return word, tuple(re.findall(r"Lb([01])E", name))


def main():
    old, new, words = bodies(sys.argv[1]), bodies(sys.argv[2]), sys.argv[3:]
    bad = 0
    for word in words:
        olds = {key(n, word): n for n in old if word in n}
        for k, n in sorted(olds.items()):
            cands = [m for m in new if word in m and key(m, word) == k]
            same = [m for m in cands if normalised(new[m]) == normalised(old[n])]
            print("%s %s: %d instructions, %s" % (word, "<%s>" % ", ".join("true" if b == "1" else "false" for b in k[1]), len(old[n]),
                                                   "identical to " + same[0] if same else "DIFFERENT from %r" % cands))
            bad += not same
        if not olds:
            print("%s: not in %s" % (word, sys.argv[1]))
            bad += 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
