#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device ISA listings (`make -C opencl-raytracer_amd/csrc asm` writes rt_wavefront.s).

    tools/isa_identity.py BEFORE.s AFTER.s > profiles/NAME.txt

A listing is split at its `.type <symbol>,@function` ... `.Lfunc_end` pairs; of every body the comments, directives and blank
lines are dropped and the function index in basic-block labels is removed (.LBB<n>_ -> .LBB_), since it only counts the
functions that precede. One line per kernel: demangled name, instructions and digest before and after. Exit status 1 if a
kernel present in both listings differs."""
import hashlib
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        text = line.split(";", 1)[0].strip()
        if not text or text.startswith(".") and not text.startswith(".LBB"):
            continue
        if text == name + ":":
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    plain = res.stdout.split("\n") if res.returncode == 0 else names
    return dict(zip(names, plain))


def digest(body):
    return hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]


def count(body):
    return sum(1 for text in body if not text.endswith(":"))


def main():
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(set(before) | set(after))
    plain = demangle(names)
    differ = 0
    print("# kernel | instructions before | digest before | instructions after | digest after | verdict")
    for n in sorted(names, key=lambda n: plain[n]):
        b, a = before.get(n), after.get(n)
        verdict = "removed" if a is None else "added" if b is None else "identical" if a == b else "DIFFERENT"
        differ += verdict == "DIFFERENT"
        print(" | ".join([plain[n], str(count(b)) if b is not None else "-", digest(b) if b is not None else "-",
                          str(count(a)) if a is not None else "-", digest(a) if a is not None else "-", verdict]))
    both = [n for n in names if n in before and n in after]
    print(f"# kernels before {len(before)}, after {len(after)}, in both {len(both)}, different {differ}")
    print(f"# instructions before {sum(count(b) for b in before.values())}, after {sum(count(a) for a in after.values())}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
