"""tools/device_code_diff.py on hand-written listings (no compiler, no GPU): what it must call identical, and what it must report."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("device_code_diff", os.path.join(ROOT, "tools", "device_code_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KERNEL = """\t.text
\t.protected\t{name}{begin}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:{at}
{bb}
\t.file\t1 "{src}"
\t.loc\t1 {line} 0
\ts_load_dword s3, s[0:1], 0x10
.LBB{n}_1:{loop}
\t{insn}
\ts_cbranch_scc1 .LBB{n}_1
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 1024
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 12
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{n}:
\t.size\t{name}, .Lfunc_end{n}-{name}
\t.set {name}.num_vgpr, {vgpr}
; NumVgprs: {vgpr}
"""
TAIL = """\t.type\t__hip_cuid_{cuid},@object
\t.globl\t__hip_cuid_{cuid}
__hip_cuid_{cuid}:
\t.byte\t0
\t.ident\t"clang {cuid}"
\t.amdgpu_metadata
---
amdhsa.kernels:
{entries}amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
\t.end_amdgpu_metadata
"""
ENTRY = """  - .agpr_count:     0
    .args:
      - .address_space:  global
        .name:           out
        .offset:         0
    .group_segment_fixed_size: 1024
    .name:           {name}
    .private_segment_fixed_size: 0
    .sgpr_count:     18
    .vgpr_count:     {vgpr}
"""


def listing(kernels, noisy=False, cuid="aaaa"):
    """kernels: [(name, instruction, vgprs)]; noisy: other comments, debug lines, cuid and label numbers around the same code"""
    text = ""
    for i, (name, insn, vgpr) in enumerate(kernels):
        text += KERNEL.format(name=name, insn=insn, vgpr=vgpr, n=i + 3 if noisy else i, src="b.hip" if noisy else "a.hip", line=90 if noisy else 7,
                              begin=" ; -- Begin function" if noisy else "", at=f" ; @{name}" if noisy else "",
                              bb="; %bb.0: ; %entry" if noisy else "; %bb.0:", loop=" ; =>This Inner Loop Header" if noisy else "")
    return text + TAIL.format(cuid="bbbb" if noisy else cuid, entries="".join(ENTRY.format(name=n, vgpr=v) for n, _, v in kernels))


BASE = [("kern_a", "v_add_f32_e32 v1, v2, v3", 24), ("kern_b", "v_mfma_f32_32x32x16_f16 v[0:15], v[16:19], v[20:23], v[0:15]", 64)]


def verdicts(parent, new):
    return {sym: (verdict, detail) for sym, verdict, detail in _tool().compare_listings(parent, new)}


def test_listings_that_differ_only_in_dropped_lines_compare_identical():
    got = verdicts(listing(BASE), listing(BASE, noisy=True))
    assert got == {"kern_a": ("identical", ""), "kern_b": ("identical", "")}


def test_a_changed_instruction_is_reported():
    new = [BASE[0], ("kern_b", "v_mfma_f32_32x32x16_f16 v[0:15], v[20:23], v[16:19], v[0:15]", 64)]
    got = verdicts(listing(BASE), listing(new, noisy=True))
    assert got["kern_a"] == ("identical", "")
    assert got["kern_b"][0] == "changed" and "v[20:23], v[16:19]" in got["kern_b"][1]


def test_a_changed_register_count_is_reported():
    new = [("kern_a", BASE[0][1], 25), BASE[1]]
    got = verdicts(listing(BASE), listing(new))
    assert got["kern_a"][0] == "changed" and "25" in got["kern_a"][1]
    assert got["kern_b"] == ("identical", "")
    # the count in the metadata alone (the code and the descriptor block unchanged)
    meta_only = listing(BASE).replace(".vgpr_count:     24", ".vgpr_count:     26")
    got = verdicts(listing(BASE), meta_only)
    assert got["kern_a"][0] == "changed" and ".vgpr_count: 26" in got["kern_a"][1]


def test_a_kernel_on_one_side_only_is_reported():
    got = verdicts(listing(BASE), listing(BASE[:1]))
    assert got == {"kern_a": ("identical", ""), "kern_b": ("only in parent", "")}
    got = verdicts(listing(BASE[1:]), listing(BASE))
    assert got == {"kern_a": ("only in new", ""), "kern_b": ("identical", "")}
