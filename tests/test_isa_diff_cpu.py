"""tools/isa_diff.py on two small assembly texts: what it must ignore (the source hash, label numbering, comment alignment, a changed name,
the text section) and what it must report (a function on one side only, a changed instruction)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_diff  # noqa: E402


def _func(name, index, body, section=None):
    return "\n".join([
        "\t.section\t.text.%s,\"axG\",@progbits,%s,comdat" % (section, section) if section else "\t.text",
        "\t.globl\t%s        ; -- Begin function %s" % (name, name),
        "\t.type\t%s,@function" % name,
        "%s:%s; @%s" % (name, " " * (40 - len(name)), name),
        "; %bb.0:"] + body + [
        ".LBB%d_1:%s; =>This Inner Loop Header: Depth=1" % (index, " " * (30 - len(str(index)))),
        "\ts_cbranch_scc1 .LBB%d_1" % index,
        "\ts_endpgm",
        "\t.section\t.rodata,\"a\",@progbits",
        "\t.amdhsa_kernel %s" % name,
        "\t\t.amdhsa_next_free_vgpr 8",
        "\t.end_amdhsa_kernel",
        "\t.section\t.text.%s,\"axG\",@progbits,%s,comdat" % (section, section) if section else "\t.text",
        ".Lfunc_end%d:" % index,
        "\t.size\t%s, .Lfunc_end%d-%s" % (name, index, name),
        "                                        ; -- End function",
        "\t.set %s.num_vgpr, 8" % name,
        "; NumVgprs: 8"]) + "\n"


def _file(tmp_path, fname, funcs, cuid):
    tail = "\t.type\t__hip_cuid_%s,@object\n__hip_cuid_%s:\n\t.amdgpu_metadata\n    .name: x\n" % (cuid, cuid)
    p = tmp_path / fname
    p.write_text("\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n" + "".join(funcs) + tail)
    return str(p)


A = ["\tv_add_f32_e32 v0, v0, v1", "\tv_mul_f32_e32 v0, v0, v2"]


def test_equal_code_under_other_labels_names_and_sections(tmp_path, capsys):
    old = _file(tmp_path, "old.s", [_func("k_gone", 0, A), _func("_Z3k_aILb0EEvv", 1, A[:1], section="_Z3k_aILb0EEvv"), _func("k_b", 2, A)], "aaaa")
    new = _file(tmp_path, "new.s", [_func("_Z3k_avv", 0, A[:1]), _func("k_b", 1, A)], "bbbb")
    assert isa_diff.main(["isa_diff", old, new]) == 0
    out = capsys.readouterr().out
    assert "only in %s: kernel k_gone (4 instructions)" % old in out
    assert "renamed, same text: kernel _Z3k_aILb0EEvv -> _Z3k_avv (3 instructions)" in out
    assert "1 identical, 1 renamed with the same text, 0 differ, 1 only in the first, 0 only in the second" in out


def test_a_changed_instruction_is_reported(tmp_path, capsys):
    old = _file(tmp_path, "old.s", [_func("k_a", 0, A), _func("k_b", 1, A)], "aaaa")
    new = _file(tmp_path, "new.s", [_func("k_a", 0, A), _func("k_b", 1, A + ["\tv_mov_b32_e32 v3, v0"])], "aaaa")
    assert isa_diff.main(["isa_diff", old, new]) == 1
    out = capsys.readouterr().out
    assert "differs: kernel k_b (4 -> 5 instructions)" in out and "1 identical" in out
