"""tools/isa_count.py on a few hand-written functions of assembly text: the instruction classes, the fields taken from the metadata, a kernel
present as two template instances under one pattern, and the exit status of --no-packed-f32.  No compiler runs here."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_count  # noqa: E402


def _func(name, index, body, kernel=True):
    return "\n".join([
        "\t.text",
        "\t.globl\t%s        ; -- Begin function %s" % (name, name),
        "\t.type\t%s,@function" % name,
        "%s:%s; @%s" % (name, " " * (40 - len(name)), name),
        "; %bb.0:"] + body + [
        ".LBB%d_1:                              ; =>This Inner Loop Header: Depth=1" % index,
        "\ts_cbranch_scc1 .LBB%d_1" % index,
        "\ts_endpgm" if kernel else "\ts_setpc_b64 s[30:31]"] + ([
        "\t.section\t.rodata,\"a\",@progbits",
        "\t.amdhsa_kernel %s" % name,
        "\t\t.amdhsa_next_free_vgpr 8",
        "\t.end_amdhsa_kernel",
        "\t.text"] if kernel else []) + [
        ".Lfunc_end%d:" % index,
        "\t.size\t%s, .Lfunc_end%d-%s" % (name, index, name),
        "                                        ; -- End function",
        "\t.set %s.num_vgpr, 8" % name,
        "; NumVgprs: 8"]) + "\n"


def _meta(entries):
    """the amdhsa.kernels list as the assembler prints it: keys in alphabetical order, the arguments nested two levels deeper"""
    out = ["\t.amdgpu_metadata", "---", "amdhsa.kernels:"]
    for name, vgpr, agpr, vspill, sspill, scratch in entries:
        out += ["  - .agpr_count:     %d" % agpr, "    .args:", "      - .name:           x", "        .offset:         0", "        .size:           8",
                "    .name:           %s" % name, "    .private_segment_fixed_size: %d" % scratch, "    .sgpr_count:     20",
                "    .sgpr_spill_count: %d" % sspill, "    .symbol:         %s.kd" % name, "    .vgpr_count:     %d" % vgpr,
                "    .vgpr_spill_count: %d" % vspill, "    .wavefront_size: 64"]
    return "\n".join(out + ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "...", "\t.end_amdgpu_metadata"]) + "\n"


CHAIN = ["\ts_load_dwordx2 s[2:3], s[0:1], 0x0",
         "\ts_waitcnt lgkmcnt(0)",
         "\tglobal_load_dwordx4 v[0:3], v8, s[2:3]",
         "\tds_read_b64_tr_b16 v[4:5], v9",
         "\ts_waitcnt vmcnt(0) lgkmcnt(0)",
         "\tv_mfma_f32_16x16x32_bf16 v[10:13], v[0:3], v[4:7], v[10:13]",
         "\tv_smfmac_f32_16x16x64_bf16 v[10:13], v[0:3], v[4:11], v14",
         "\tv_fma_f32 v0, v1, v2, v3",
         "\tv_fmac_f32_e32 v0, v1, v2",
         "\tv_cvt_pk_bf16_f32 v0, v1, v2",
         "\tv_pk_mov_b32 v[0:1], v[2:3], v[4:5]",
         "\tv_accvgpr_write_b32 a0, v0",
         "\ts_nop 1",
         "\ts_barrier",
         "\tds_write_b32 v9, v0",
         "\tglobal_store_dword v8, v0, s[2:3]",
         "\tglobal_atomic_add_f32 v8, v0, s[2:3]",
         "\tscratch_load_dword v1, off, off offset:4",
         "\tbuffer_load_dword v1, v2, s[4:7], 0 offen",
         "\tflat_load_dword v1, v[2:3]",
         "\ts_add_u32 s4, s4, 1"]
PACKED = ["\tv_pk_fma_f32 v[4:5], v[0:1], v[4:5], v[8:9]", "\tv_pk_add_f32 v[0:1], v[0:1], v[4:5]", "\tv_pk_mul_f32 v[0:1], v[0:1], v[4:5] op_sel_hi:[1,0]"]
OCC8, OCC4, ADAM = "_Z22k_decode_fwd_multi_occILi8EEv9MultiArgs", "_Z22k_decode_fwd_multi_occILi4EEv9MultiArgs", "_Z12k_adam_multi8AdamArgs"


def _file(tmp_path, packed_in_occ4=False):
    text = ("\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n"
            + _func(OCC8, 0, CHAIN)
            + _func("_Z6helperv", 1, PACKED, kernel=False)                                     # a function that is no kernel is not listed
            + _func(OCC4, 2, CHAIN[:8] + (PACKED[:1] if packed_in_occ4 else []))
            + _func(ADAM, 3, PACKED + CHAIN[7:9])
            + "\t.type\t__hip_cuid_abcd,@object\n__hip_cuid_abcd:\n"
            + _meta([(OCC8, 225, 4, 0, 0, 0), (OCC4, 128, 0, 13, 2, 52), (ADAM, 24, 0, 0, 0, 0)]))
    p = tmp_path / "dev.s"
    p.write_text(text)
    return str(p)


def test_classes_and_metadata(tmp_path):
    rows = isa_count.census(_file(tmp_path))
    assert list(rows) == [OCC8, OCC4, ADAM]
    r = rows[OCC8]
    want = dict(matrix=2, packed_f32=0, vector=5, lds=2, global_load=1, global_store=1, global_atomic=1, other_mem=3, scalar=4, waits=4, other=0)
    assert {c: r[c] for c in isa_count.CLASSES} == want                # scalar: s_load, s_add, s_cbranch, s_endpgm; waits: 2 s_waitcnt, s_nop, s_barrier
    assert r["total"] == len(CHAIN) + 2 == sum(want.values())
    assert (r["vgpr"], r["agpr"], r["vgpr_spill"], r["sgpr_spill"], r["scratch_bytes"]) == (225, 4, 0, 0, 0)
    r = rows[OCC4]
    assert (r["vgpr"], r["agpr"], r["vgpr_spill"], r["sgpr_spill"], r["scratch_bytes"]) == (128, 0, 13, 2, 52)
    r = rows[ADAM]
    assert (r["packed_f32"], r["vector"], r["matrix"], r["total"]) == (3, 2, 0, 7)
    for m, c in (("v_pk_fma_f32", "packed_f32"), ("v_pk_add_f32_e64", "packed_f32"), ("v_pk_fma_f16", "vector"), ("v_cvt_pk_bf16_f32", "vector"),
                 ("v_mfma_f32_32x32x2_f32", "matrix"), ("s_waitcnt_vscnt", "waits"), ("s_cbranch_vccnz", "scalar"), ("global_load_lds_dwordx4", "global_load")):
        assert isa_count.classify(m) == c, m


def test_one_pattern_lists_both_template_instances_and_the_guard_decides_the_exit_status(tmp_path, capsys):
    clean = _file(tmp_path)
    assert isa_count.main(["isa_count", clean, "--no-packed-f32", "k_decode_"]) == 0
    out = capsys.readouterr().out
    assert OCC8 in out and OCC4 in out and ADAM not in out and "helper" not in out
    assert isa_count.main(["isa_count", clean, "k_adam"]) == 0                                  # packed f32 in a kernel nobody guards is only counted
    assert ADAM in capsys.readouterr().out
    assert isa_count.main(["isa_count", clean, "--no-packed-f32", "k_adam_multi"]) == 1
    assert "3 packed f32 instructions in " + ADAM in capsys.readouterr().out
    assert isa_count.main(["isa_count", clean, "--no-packed-f32", "k_no_such_kernel"]) == 1    # a guard that guards nothing is a mistake
    capsys.readouterr()
    dirty = _file(tmp_path, packed_in_occ4=True)
    assert isa_count.main(["isa_count", dirty, "k_adam", "--no-packed-f32", "k_decode_fwd_multi_occ"]) == 1
    out = capsys.readouterr().out
    assert "1 packed f32 instructions in " + OCC4 in out and "instructions in " + OCC8 not in out and ADAM in out
