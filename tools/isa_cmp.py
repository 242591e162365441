"""Compare the per-kernel gfx950 assembly of two trees of this repository.

Every device source file (csrc/*.hip) of both trees is compiled to assembly with the product's
flags (tools/hazard_scan.compile_all), split into kernels (a kernel = a function with a
.amdhsa_kernel descriptor: its instructions and that descriptor, so a kernarg size or a register
count that moves shows too), and the listings are compared after dropping comments and
normalising local labels and the kernel's own symbol name.  Per file it prints the kernel counts,
every kernel that is NEW, GONE or DIFF (with listing lines old / new), and ORDER when the common
kernels are emitted in another order (identical kernels at other addresses in the code object:
instruction-cache alignment can move a timing by a few tenths of a percent); exit status 1 when
anything is listed.  It only diffs: what the kernels contain is hazard_scan's business.

    python tools/isa_cmp.py OLD_TREE [NEW_TREE]     # NEW_TREE defaults to this checkout
    git worktree add /tmp/parent HEAD~1 && python tools/isa_cmp.py /tmp/parent
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hazard_scan  # noqa: E402

LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp)\d+(_\d+)?")


def kernels(path):
    """{mangled name: [normalised listing lines]} of every kernel in an assembly file."""
    body, desc, cur, in_desc = {}, {}, None, None
    for raw in open(path):
        l = raw.split(";")[0].rstrip()
        if not l.strip():
            continue
        s = l.strip()
        m = hazard_scan.FUNC.match(s)
        if m:
            cur = m.group(1)
            body[cur] = []
            continue
        if s.startswith(".amdhsa_kernel "):
            in_desc = s.split()[1]
            desc[in_desc] = []
            continue
        if s == ".end_amdhsa_kernel":
            in_desc = None
            continue
        if in_desc:
            desc[in_desc].append(s)
        elif cur:
            if s.startswith(".Lfunc_end"):
                cur = None
            elif not s.startswith((".p2align", ".section", ".type", ".size", ".globl", ".protected", ".weak")):
                body[cur].append(s)
    out = {}
    for name in body:   # in the order the functions are emitted: their layout in the code object
        if name not in desc:
            continue
        lines = body[name] + desc[name]
        out[name] = [LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), x).replace(name, "<self>")
                     for x in lines]
    return out


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or not filt:
        return {n: n for n in names}
    out = subprocess.run([filt, *names], capture_output=True, text=True, check=True).stdout.splitlines()
    short = [re.sub(r"^void |\(.*$", "", o).replace("(anonymous namespace)", "anon") for o in out]
    return dict(zip(names, short))


def compile_tree(tree, outdir):
    files = hazard_scan.compile_all(outdir, root=os.path.abspath(tree))
    return {os.path.basename(f)[:-2]: kernels(f) for f in files}


def main(argv):
    if not 1 <= len(argv) <= 2:
        print(__doc__)
        return 2
    old_tree, new_tree = argv[0], argv[1] if len(argv) > 1 else hazard_scan.ROOT
    with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
        old, new = compile_tree(old_tree, da), compile_tree(new_tree, db)
    listed = 0
    for f in sorted(set(old) | set(new)):
        a, b = old.get(f, {}), new.get(f, {})
        if not a and not b:
            continue   # host code only
        print(f"== {f}: old {len(a)} kernels, new {len(b)}")
        names = demangle(sorted(set(a) | set(b)))
        for n in sorted(set(a) | set(b), key=lambda n: names[n]):
            if n not in a:
                print(f"  NEW  {len(b[n]):7d}  {names[n]}")
            elif n not in b:
                print(f"  GONE {len(a[n]):7d}  {names[n]}")
            elif a[n] != b[n]:
                print(f"  DIFF {len(a[n]):7d} / {len(b[n]):7d}  {names[n]}")
            else:
                continue
            listed += 1
        if [n for n in a if n in b] != [n for n in b if n in a]:
            print("  ORDER  the common kernels are emitted in another order")
            listed += 1
    print(f"kernels new, gone or different, files reordered: {listed}")
    return 1 if listed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
