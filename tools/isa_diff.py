#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel (host only, no GPU).

    make -C nice-slam-cpp_amd/csrc asm          # in each tree: csrc/nsk_gfx950.s, from the library's own flags
    python tools/isa_diff.py OLD.s NEW.s

Each file is split at the assembler's "-- Begin function" markers.  A function's text runs to the next marker: its instructions, its kernel
descriptor (.amdhsa_kernel: registers, LDS, scratch) and the compiler's resource summary.  Before two texts are compared
  * lines that contain __hip_cuid_ are dropped (that symbol is a hash of the source text),
  * local labels (.LBB12_3, .Lfunc_end12, .LJTI12_0, .Ltmp7; BB12_3 in comments) are renumbered in order of appearance, since they carry the
    function's index in the file, which moves when a function in front of it is added or removed, and runs of blanks become one blank (the
    assembler aligns the comments behind labels of different lengths),
  * the function's own name is replaced by a placeholder, so that a kernel whose mangled name changed (a template parameter dropped) still
    pairs with its former self: functions present on one side only whose texts are equal are reported as renamed, not as missing.  For the
    same reason every switch to a text section reads ".text": a template instance lives in a comdat section named after it, a plain kernel
    in .text.
Prints the functions on one side only, the renamed ones, and those whose text differs with their instruction counts.  Exit status 1 when any
function differs, else 0."""
import re
import sys

BEGIN = re.compile(r"--\s*Begin function (\S+)")
TAIL = re.compile(r"^\s*\.(type\s+__hip_cuid_|amdgpu_metadata|ident\b)")
LOCAL = re.compile(r"\.L[A-Za-z_$.]*\d+(?:_\d+)?|\bBB\d+_\d+\b")
TEXT = re.compile(r"^\s*\.(text\b|section\s+\.text)")
INSTR = re.compile(r"^\s+[a-z][a-z0-9_]*(\s|$)")


def functions(path):
    """[(name, raw lines)] in file order: a function's lines run from its "-- Begin function" marker to the next marker or the file's tail"""
    out, name, lines = [], None, []
    with open(path) as f:
        for ln in f:
            m = BEGIN.search(ln)
            if m or TAIL.match(ln):
                if name is not None:
                    out.append((name, lines))
                name, lines = (m.group(1) if m else None), []
            if name is not None:
                lines.append(ln)
    if name is not None:
        out.append((name, lines))
    return out


def body(lines):
    """the lines in front of the function's end label: its instructions, without the descriptor and the resource summary"""
    return lines[: next((i for i, ln in enumerate(lines) if ".Lfunc_end" in ln and ln.rstrip().endswith(":")), len(lines))]


def split(path):
    """{name: (is_kernel, instruction count, normalised text)} in file order"""
    funcs = {}
    for name, lines in functions(path):
        table = {}

        def renumber(m):
            key = m.group(0)
            key = key if key.startswith(".L") else ".L" + key
            return table.setdefault(key, ".L%d" % len(table))

        while lines and TEXT.match(lines[-1]):          # the section switch in front of the NEXT function's marker
            lines.pop()
        text = [".text" if TEXT.match(ln) else " ".join(LOCAL.sub(renumber, ln).replace(name, "<self>").split()) for ln in lines if "__hip_cuid_" not in ln]
        funcs[name] = (any(".amdhsa_kernel" in ln for ln in lines), sum(1 for ln in body(lines) if INSTR.match(ln)), "\n".join(text))
    return funcs


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = split(argv[1]), split(argv[2])
    kind = lambda f: "kernel" if f[0] else "function"
    only_a, only_b = [n for n in a if n not in b], [n for n in b if n not in a]
    renamed = []
    for n in list(only_a):
        twin = next((m for m in only_b if b[m][2] == a[n][2]), None)
        if twin:
            renamed.append((n, twin))
            only_a.remove(n)
            only_b.remove(twin)
    differ = [n for n in a if n in b and a[n][2] != b[n][2]]
    print("%s: %d kernels, %d other functions" % (argv[1], sum(f[0] for f in a.values()), sum(not f[0] for f in a.values())))
    print("%s: %d kernels, %d other functions" % (argv[2], sum(f[0] for f in b.values()), sum(not f[0] for f in b.values())))
    for n in only_a:
        print("only in %s: %s %s (%d instructions)" % (argv[1], kind(a[n]), n, a[n][1]))
    for n in only_b:
        print("only in %s: %s %s (%d instructions)" % (argv[2], kind(b[n]), n, b[n][1]))
    for n, m in renamed:
        print("renamed, same text: %s %s -> %s (%d instructions)" % (kind(a[n]), n, m, a[n][1]))
    for n in differ:
        print("differs: %s %s (%d -> %d instructions)" % (kind(a[n]), n, a[n][1], b[n][1]))
    print("%d identical, %d renamed with the same text, %d differ, %d only in the first, %d only in the second"
          % (sum(1 for n in a if n in b) - len(differ), len(renamed), len(differ), len(only_a), len(only_b)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
