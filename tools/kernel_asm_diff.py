"""Compare the device assembly of kernels between two builds, kernel by kernel, apart from symbol and file names.

    hipcc <build.py's FLAGS> --cuda-device-only -S old/raster.hip -o old.s      (one .s per source, both sides)
    python tools/kernel_asm_diff.py old.s new1.s [new2.s ...] -- "k_bin<true>=k_bin<true>" "k_setup<true, true>=k_setup<sah::MotionAttr>" [-v]
    python tools/kernel_asm_diff.py old.s new.s [-v]

Each pair names one kernel of the first file and one of the others by a substring of its demangled name; without the list every kernel of
the first file is compared with the kernel of the same demangled name in the others, and a kernel that only one side has is a failure.
The exit status is non-zero when any kernel differs or is missing.  Compared is the text from the
kernel's label to its .Lfunc_end (instructions, kernel descriptor, resource directives) with the kernel's own symbol, the function number
in .LBB<n>_ labels and assembler comments masked.  For a kernel that differs, the second figure says whether the two texts are the same
multiset of lines once the operands of every instruction are sorted (commuted operands, reordered instructions); -v prints the diff."""
import collections
import difflib
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        sym, body = m.group(1), m.group(2)
        if ".amdhsa_kernel " + sym not in body:
            continue  # a device function, not a kernel
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = re.sub(r"^\s*;.*\n", "", body, flags=re.M)
        body = re.sub(r"\s*;.*$", "", body, flags=re.M)
        name = subprocess.run(["c++filt", sym], stdout=subprocess.PIPE, text=True).stdout.strip()
        out[name] = body.replace(sym, "SYM").splitlines()
    return out


def sorted_operands(line):
    parts = re.split(r"[ ,\t]+", line.strip())
    return (parts[0], tuple(sorted(parts[1:])))


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    sep = args.index("--") if "--" in args else len(args)
    old, new = kernels(args[0]), {}
    for p in args[1:sep]:
        new.update(kernels(p))
    failed = False
    if sep == len(args):  # no list: every kernel against the one of the same demangled name; a kernel of one side only is a failure
        for k in sorted(set(old) ^ set(new)):
            print(f"MISSING    only in the {'old' if k in old else 'new'} build  {k}")
            failed = True
        pairs = [(k, k, k, k) for k in sorted(set(old) & set(new))]
    else:
        pairs = []
        for pair in args[sep + 1:]:
            a, b = pair.split("=")
            ka, kb = [k for k in old if a in k], [k for k in new if b in k]
            assert len(ka) == 1 and len(kb) == 1, (pair, ka, kb)
            pairs.append((a, b, ka[0], kb[0]))
    for a, b, ka, kb in pairs:
        la, lb = old[ka], new[kb]
        if la == lb:
            print(f"identical  {len(la):6d} lines  {a}  ->  {b}")
            continue
        failed = True
        differing = sum(1 for o in difflib.SequenceMatcher(None, la, lb, autojunk=False).get_opcodes() if o[0] != "equal" for _ in range(max(o[2] - o[1], o[4] - o[3])))
        same = collections.Counter(map(sorted_operands, la)) == collections.Counter(map(sorted_operands, lb))
        print(f"DIFFERENT  {len(la):6d} -> {len(lb)} lines, {differing} differ, same multiset with sorted operands: {'yes' if same else 'no'}  {a}  ->  {b}")
        if "-v" in sys.argv:
            for line in difflib.unified_diff(la, lb, lineterm="", n=1):
                print("    " + line)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
