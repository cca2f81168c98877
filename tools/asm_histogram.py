#!/usr/bin/env python3
"""Per-kernel histogram of the waits and memory instructions in a device assembly file (hipcc --save-temps:
<source>-hip-amdgcn-amd-amdhsa-gfx950.s).

A weight-streaming loop lives on its counted waits: a wait that comes out as vmcnt(1) where the steady state is
vmcnt(D - 1) drains the prefetch ring, and only the assembly shows it.  One line per kernel and key, so that two builds
are compared with `diff`:

    python tools/asm_histogram.py gemv_f32-hip-amdgcn-amd-amdhsa-gfx950.s [--kernel REGEX] [--out FILE]

Keys: every vmcnt(N) / lgkmcnt(N) / expcnt(N) operand of an s_waitcnt (a combined wait counts once under each of its
operands) and the instructions in COUNTED (a trailing * takes every mnemonic with that prefix).
"""
import argparse
import collections
import re
import sys

COUNTED = ["global_load_dwordx4", "global_load_dword", "global_store_*", "v_mfma_*", "ds_read_b128", "ds_write_b128", "s_barrier"]


def key_of(mnemonic):
    for c in COUNTED:
        if mnemonic == c or (c.endswith("*") and mnemonic.startswith(c[:-1])):
            return c
    return None


def histogram(path, kernel_rx):
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M))
    out, cur = collections.OrderedDict(), None
    for line in open(path):
        line = line.split(";")[0].strip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):$", line)
        if m and m.group(1) in kernels:
            cur = out.setdefault(m.group(1), collections.Counter()) if re.search(kernel_rx, m.group(1)) else None
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not line or line.startswith("."):
            continue
        mnemonic, _, operands = line.partition(" ")
        if mnemonic == "s_waitcnt":
            for part in re.findall(r"(?:vmcnt|lgkmcnt|expcnt)\(\d+\)", operands):
                cur["s_waitcnt " + part] += 1
        elif key_of(mnemonic):
            cur[key_of(mnemonic)] += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default=".", help="regex on the (mangled) kernel symbol")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []
    for name, h in sorted(histogram(a.asm, a.kernel).items()):
        for k in sorted(h, key=lambda k: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", k)]):
            lines.append("%s  %-28s %5d" % (name, k, h[k]))
        lines.append("")
    if not lines:
        sys.exit("no kernel in %s matches %r" % (a.asm, a.kernel))
    text = "\n".join(lines)
    if a.out:
        open(a.out, "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
