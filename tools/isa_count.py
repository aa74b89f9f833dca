#!/usr/bin/env python3
"""Instruction census of the device code, kernel by kernel (host only, no GPU).

    make -C nice-slam-cpp_amd/csrc asm
    python tools/isa_count.py nice-slam-cpp_amd/csrc/nsk_gfx950.s [kernel-name-pattern ...] [--no-packed-f32 PATTERN ...]

The file is split into functions as tools/isa_diff.py splits it.  For every kernel whose (mangled) name matches one of the patterns (regular
expressions, searched; none given: every kernel) one line: the instruction total and the instructions per class, by mnemonic family only --
  matrix      v_mfma_*, v_smfmac_*
  packed f32  v_pk_*_f32 (v_pk_fma_f32, v_pk_add_f32, v_pk_mul_f32): beside MFMAs each costs more than the two single instructions it
              stands for
  vector      every other v_*
  LDS         ds_*
  global      global_load* / global_store* / global_atomic*, three columns
  other mem   buffer_*, flat_*, scratch_* (scratch_* is what a register spill reads and writes)
  scalar      every other s_*
  waits       s_waitcnt*, s_nop, s_sleep, s_barrier
-- and, from the .amdgpu_metadata entry of the kernel, its VGPR count, AGPR count, spilled VGPRs and SGPRs and scratch bytes.  A template
instance is a kernel of its own name: one pattern may list several.

--no-packed-f32 PATTERN (repeatable): the kernels matching PATTERN are listed too, and the exit status is 1 when one of them contains a
packed f32 instruction (or when PATTERN matches no kernel), else 0."""
import re
import sys

import isa_diff

MNEMONIC = re.compile(r"^\s+([a-z][a-z0-9_]*)(?:\s|$)")
CLASSES = ("matrix", "packed_f32", "vector", "lds", "global_load", "global_store", "global_atomic", "other_mem", "scalar", "waits", "other")
SHORT = {"packed_f32": "pk_f32", "global_load": "g_load", "global_store": "g_store", "global_atomic": "g_atomic", "other_mem": "oth_mem",
         "vgpr_spill": "v_spill", "sgpr_spill": "s_spill", "scratch_bytes": "scratch"}          # column heads of the printed table
WAITS = re.compile(r"s_(waitcnt\w*|nop|sleep|barrier)$")
PACKED_F32 = re.compile(r"v_pk_\w+_f32(_|$)")
META_KEYS = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".vgpr_spill_count": "vgpr_spill", ".sgpr_spill_count": "sgpr_spill",
             ".private_segment_fixed_size": "scratch_bytes"}


def classify(m):
    """the class of one mnemonic"""
    if m.startswith(("v_mfma_", "v_smfmac_")):
        return "matrix"
    if PACKED_F32.match(m):
        return "packed_f32"
    if m.startswith("v_"):
        return "vector"
    if m.startswith("ds_"):
        return "lds"
    for kind in ("load", "store", "atomic"):
        if m.startswith("global_" + kind):
            return "global_" + kind
    if m.startswith(("buffer_", "flat_", "scratch_")):
        return "other_mem"
    if WAITS.match(m):
        return "waits"
    if m.startswith("s_"):
        return "scalar"
    return "other"


def metadata(path):
    """{kernel name: {vgpr, agpr, vgpr_spill, sgpr_spill, scratch_bytes}} from the amdhsa.kernels list of .amdgpu_metadata"""
    out, cur, inside = {}, None, False

    def close():
        if cur and ".symbol" in cur:
            name = cur.pop(".symbol")
            out[name[:-3] if name.endswith(".kd") else name] = cur

    with open(path) as f:
        for ln in f:
            if ln.lstrip().startswith(".amdgpu_metadata"):
                inside = True
            elif ln.lstrip().startswith(".end_amdgpu_metadata"):
                inside = False
            if not inside:
                continue
            m = re.match(r"^  (- | {2})(\.\w+):\s*(\S*)", ln)        # a key of a kernel entry: indent 4, the entry's first behind "  - "
            if not m:
                continue
            if m.group(1) == "- ":
                close()
                cur = {}
            if cur is None:
                continue
            if m.group(2) == ".symbol":
                cur[".symbol"] = m.group(3).strip("'\"")
            elif m.group(2) in META_KEYS:
                cur[META_KEYS[m.group(2)]] = int(m.group(3))
    close()
    return out


def census(path):
    """{kernel name: {"total", every class, the metadata fields (None where the file has none)}} in file order"""
    meta, out = metadata(path), {}
    for name, lines in isa_diff.functions(path):
        if not any(".amdhsa_kernel" in ln for ln in lines):
            continue
        row = dict.fromkeys(CLASSES, 0)
        for ln in isa_diff.body(lines):
            m = MNEMONIC.match(ln)
            if m:
                row[classify(m.group(1))] += 1
        row["total"] = sum(row[c] for c in CLASSES)
        for k in META_KEYS.values():
            row[k] = meta.get(name, {}).get(k)
        out[name] = row
    return out


def main(argv):
    args, patterns, guarded = argv[1:], [], []
    while args:
        a = args.pop(0)
        if a == "--no-packed-f32":
            if not args:
                print(__doc__)
                return 2
            guarded.append(args.pop(0))
        else:
            patterns.append(a)
    if not patterns or patterns[0].startswith("-"):
        print(__doc__)
        return 2
    rows = census(patterns.pop(0))
    hit = lambda name, pats: any(re.search(p, name) for p in pats)
    shown = [n for n in rows if hit(n, patterns + guarded) or not (patterns or guarded)]
    cols = ("total",) + CLASSES + tuple(META_KEYS.values())
    print(" ".join("%8s" % SHORT.get(c, c) for c in cols) + "  kernel")
    for n in shown:
        print(" ".join("%8s" % ("-" if rows[n][c] is None else rows[n][c]) for c in cols) + "  " + n)
    status = 0
    for p in guarded:
        names = [n for n in rows if re.search(p, n)]
        if not names:
            print("--no-packed-f32 %s: no kernel matches" % p)
            status = 1
        for n in names:
            if rows[n]["packed_f32"]:
                print("--no-packed-f32 %s: %d packed f32 instructions in %s" % (p, rows[n]["packed_f32"], n))
                status = 1
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv))
