"""CPU: scripts/kernel_asm_diff.py compares two builds' kernels, on synthetic assembly text.

The tool is how a refactor of the kernel sources shows that no kernel's code changed
(`make asm` in both trees, then the tool on the two build directories). No compiler here:
a few lines in the shape hipcc writes, a plain kernel and a template instance (whose
descriptor block comes before its .Lfunc_end label).
"""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location(
    "kernel_asm_diff", os.path.join(ROOT, "scripts", "kernel_asm_diff.py"))
kad = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kad)


def plain(name, ordinal, reg="v1", comment="; %bb.0:"):
    return """
\t.globl\t{n}
{n}: ; @{n}
{c}
\ts_load_dword s3, s[0:1], 0x90
\tv_add_u32_e32 {r}, s2, v0
\ts_cbranch_execz .LBB{o}_2
.LBB{o}_2:                              ; %Flow7
\ts_endpgm
.Lfunc_end{o}:
\t.size\t{n}, .Lfunc_end{o}-{n}
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {n}
\t\t.amdhsa_next_free_vgpr 14
\t.end_amdhsa_kernel
\t.text
""".format(n=name, o=ordinal, r=reg, c=comment)


def instance(name, ordinal, vgprs=58):
    return """
\t.section\t.text.{n},"axG",@progbits,{n},comdat
{n}: ; @{n}
\ts_branch .LBB{o}_1
.LBB{o}_1:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {n}
\t\t.amdhsa_next_free_vgpr {v}
\t.end_amdhsa_kernel
\t.section\t.text.{n},"axG",@progbits,{n},comdat
.Lfunc_end{o}:
\t.size\t{n}, .Lfunc_end{o}-{n}
""".format(n=name, o=ordinal, v=vgprs)


def write(tmp_path, side, files):
    d = tmp_path / side
    d.mkdir()
    for name, text in files.items():
        (d / name).write_text(text)
    return str(d)


def test_label_ordinals_comments_and_unit_cut_do_not_count(tmp_path, capsys):
    old = write(tmp_path, "old", {"all.s": plain("k_a", 0) + plain("k_b", 1) + instance("k_cILi58EE", 2),
                                  "host.s": "main:\n\tretq\n"})
    new = write(tmp_path, "new", {"u1.s": plain("k_b", 0, comment="; %entry"),
                                  "u2.s": instance("k_cILi58EE", 0) + plain("k_a", 1)})
    assert kad.main([old, new]) == 0
    assert capsys.readouterr().out.strip().endswith("0 on one side only, 0 differ")
    both = kad.kernels_in(new)
    assert sorted(both) == ["k_a", "k_b", "k_cILi58EE"]
    assert "\tv_add_u32_e32 v1, s2, v0" in both["k_a"]          # trailing blanks dropped
    assert "\t\t.amdhsa_next_free_vgpr 58" in both["k_cILi58EE"]  # the descriptor block too


def test_changed_register_is_reported(tmp_path, capsys):
    old = write(tmp_path, "old", {"a.s": plain("k_a", 0) + plain("k_b", 1)})
    new = write(tmp_path, "new", {"a.s": plain("k_a", 0) + plain("k_b", 1, reg="v2")})
    assert kad.compare(kad.kernels_in(old), kad.kernels_in(new)) == ([], [], ["k_b"])
    assert kad.main([old, new]) == 1
    out = capsys.readouterr().out
    assert "differs: k_b" in out and "+\tv_add_u32_e32 v2, s2, v0" in out
    assert out.strip().endswith("0 on one side only, 1 differ")


def test_changed_descriptor_is_reported(tmp_path):
    old = write(tmp_path, "old", {"a.s": instance("k_cILi58EE", 0)})
    new = write(tmp_path, "new", {"a.s": instance("k_cILi58EE", 0, vgprs=60)})
    assert kad.compare(kad.kernels_in(old), kad.kernels_in(new)) == ([], [], ["k_cILi58EE"])


def test_missing_kernel_is_reported(tmp_path, capsys):
    old = write(tmp_path, "old", {"a.s": plain("k_a", 0) + plain("k_b", 1)})
    new = write(tmp_path, "new", {"a.s": plain("k_a", 0), "b.s": plain("k_new", 0)})
    assert kad.compare(kad.kernels_in(old), kad.kernels_in(new)) == (["k_b"], ["k_new"], [])
    assert kad.main([old, new]) == 1
    out = capsys.readouterr().out
    assert "only in %s: k_b" % old in out and "only in %s: k_new" % new in out
    assert out.strip().endswith("2 on one side only, 0 differ")
