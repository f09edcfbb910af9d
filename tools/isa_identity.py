#!/usr/bin/env python3
"""Are the kernels of two checkouts of this repository the same machine code?

    python tools/isa_identity.py BEFORE_TREE AFTER_TREE > profiles/refactor_isa_identity.txt

For a refactor that must not change a kernel.  Every csrc/*.hip of both trees is compiled to device assembly with
the exact command its Makefile gives for the object (`make -n`, so per-file flags are included) plus
--cuda-device-only -S.  The output is split by function symbol (the kernels, and any device function that was not
inlined); file and line directives, comments and the numbering of local labels (which depends on a function's
position in its file) are dropped.  One line per symbol: the file it
lives in before, the file after, and whether instruction stream and .amdhsa_ resource lines are identical.
Exit status 1 if a symbol differs or exists on one side only.
"""
import concurrent.futures
import glob
import os
import re
import shlex
import subprocess
import sys
import tempfile


def device_asm(tree, src, out):
    pkg = os.path.join(tree, "d-liom_amd")
    obj = src[:-4] + ".o"
    dry = subprocess.run(["make", "-C", pkg, "-n", "-B", obj], check=True, capture_output=True, text=True).stdout
    cmd = next(shlex.split(l) for l in dry.splitlines() if " -c " in l and src in l)
    cmd = [a for a in cmd[:cmd.index("-o")] if a != "-c"] + ["--cuda-device-only", "-S", "-o", out]
    subprocess.run(cmd, cwd=pkg, check=True)


def kernels(asm_path):
    """{function symbol (kernels and whatever was not inlined into them): (instruction lines, .amdhsa_ lines)}"""
    text = open(asm_path).read()
    out = {}
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        lines, desc = [], []
        for l in m.group(2).splitlines():
            l = l.split(";")[0].strip()
            if ".amdhsa_" in l:
                desc.append(l)
            elif l and not l.startswith((".loc", ".file", ".cfi_", ".p2align", ".section", ".text")):
                lines.append(re.sub(r"\.L(BB|tmp|JTI)\d+_", r".L\1_", l))
        out[m.group(1)] = (lines, desc)
    return out


def tree_kernels(tree, tmp, tag):
    srcs = sorted(os.path.relpath(p, os.path.join(tree, "d-liom_amd")) for p in glob.glob(os.path.join(tree, "d-liom_amd/csrc/*.hip")))
    outs = {s: os.path.join(tmp, "%s_%s.s" % (tag, os.path.basename(s))) for s in srcs}
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda s: device_asm(tree, s, outs[s]), srcs))
    found = {}
    for s in srcs:
        for name, k in kernels(outs[s]).items():
            found[name] = (s, k)
    return found


def main():
    before_tree, after_tree = sys.argv[1:3]
    with tempfile.TemporaryDirectory() as tmp:
        before, after = tree_kernels(before_tree, tmp, "before"), tree_kernels(after_tree, tmp, "after")
    bad, third_party = 0, {}
    print("# kernel | file before | file after | instructions and .amdhsa_ lines identical")
    for name in sorted(set(before) | set(after)):
        b, a = before.get(name), after.get(name)
        same = b is not None and a is not None and b[1] == a[1]
        bad += not same
        if same and name.startswith("_ZN7rocprim"):  # hipcub's instantiations: hundreds of them, one line per file
            third_party[(b[0], a[0])] = third_party.get((b[0], a[0]), 0) + 1
            continue
        print("%s | %s | %s | %s" % (name, b[0] if b else "-", a[0] if a else "-", "yes" if same else "NO"))
    for (b, a), count in sorted(third_party.items()):
        print("(%d rocprim instantiations) | %s | %s | yes" % (count, b, a))
    print("# %d symbols, %d differ" % (len(set(before) | set(after)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
