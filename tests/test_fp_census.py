"""tools/fp_census.py's parser on a short synthetic listing: per-line (fused, mul, add)
triples, the diff of two listings, the copy-count marking and the line map.  Nothing is
compiled here (a kernel compile takes about a minute)."""

import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("fp_census", os.path.join(ROOT, "tools", "fp_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FC = _tool()

LISTING_A = """\
\t.text
\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.file\t1 "/src/csrc" "dx_step.hip"
\t.protected\t_Z7kernelAv
\t.globl\t_Z7kernelAv
\t.p2align\t8
\t.type\t_Z7kernelAv,@function
_Z7kernelAv:
.Lfunc_begin0:
\t.loc\t1 10 0
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\t.file\t2 "/src/csrc/dx_device.h"
\t.loc\t2 20 5 prologue_end
\tv_mul_f32_e32 v1, v0, v0
\tv_fma_f32 v2, v1, v0, v1
\tv_add_f32_e64 v3, v2, s0
\t.loc\t2 21 9
\tv_fmac_f32_e32 v3, v1, v2
\tv_fmac_f32_dpp v3, v1, v2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf
\tv_add_u32_e32 v9, v3, v2
\tv_fma_f64 v[10:11], v[4:5], v[6:7], v[8:9]
\ts_cbranch_execz .LBB0_2
.LBB0_1:
\t.p2align\t4
\t.loc\t1 30 3 is_stmt 0
\tv_pk_mul_f32 v[4:5], v[0:1], v[2:3]
\tv_pk_fma_f32 v[4:5], v[0:1], v[2:3], v[4:5]
\tv_sub_f32_e32 v6, v4, v5
\tv_subrev_f32_dpp v6, v4, v5 row_shr:1 row_mask:0xf bank_mask:0xf
.LBB0_2:
\t.loc\t2 20 5
\tv_mul_f32_e64 v1, s2, v0
\t; a comment: v_mul_f32_e32 v0, v0, v0
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z7kernelAv, .Lfunc_end0-_Z7kernelAv
\t.amdhsa_kernel _Z7kernelAv
\t.end_amdhsa_kernel
\t.type\t_Z7kernelBv,@function
_Z7kernelBv:
.Lfunc_begin1:
\t.loc\t1 40 1
\tv_mul_f32_e32 v1, v0, v0
\tv_add_f32_e32 v2, v1, v0
\tv_mul_f32_e32 v3, v0, v0
\tv_add_f32_e32 v4, v3, v0
\t.loc\t1 50 1
\tv_fmaak_f32 v5, v0, v1, 0x40000000
\ts_endpgm
.Lfunc_end1:
\t.amdhsa_kernel _Z7kernelBv
\t.end_amdhsa_kernel
"""

# kernel A: line 20 of dx_device.h loses its fusion (fma -> mul + add); line 30 of
# dx_step.hip holds two copies.  kernel B: one copy of line 40 vanished, line 50 moved to 53.
LISTING_B = (
    LISTING_A
    .replace("\tv_fma_f32 v2, v1, v0, v1\n", "\tv_mul_f32_e32 v2, v1, v0\n\tv_add_f32_e32 v2, v2, v1\n")
    .replace("\tv_pk_mul_f32 v[4:5], v[0:1], v[2:3]\n\tv_pk_fma_f32 v[4:5], v[0:1], v[2:3], v[4:5]\n"
             "\tv_sub_f32_e32 v6, v4, v5\n\tv_subrev_f32_dpp v6, v4, v5 row_shr:1 row_mask:0xf bank_mask:0xf\n",
             2 * ("\tv_pk_mul_f32 v[4:5], v[0:1], v[2:3]\n\tv_pk_fma_f32 v[4:5], v[0:1], v[2:3], v[4:5]\n"
                  "\tv_sub_f32_e32 v6, v4, v5\n\tv_subrev_f32_dpp v6, v4, v5 row_shr:1 row_mask:0xf bank_mask:0xf\n"))
    .replace("\tv_mul_f32_e32 v3, v0, v0\n\tv_add_f32_e32 v4, v3, v0\n", "")
    .replace("\t.loc\t1 50 1\n", "\t.loc\t1 53 1\n")
)


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_classes():
    assert FC.fp_class("v_fma_f32") == 0 and FC.fp_class("v_fmac_f32_e64_dpp") == 0 and FC.fp_class("v_pk_fma_f32") == 0
    assert FC.fp_class("v_mul_f32_e64") == 1 and FC.fp_class("v_pk_mul_f32") == 1
    assert FC.fp_class("v_add_f32_dpp") == 2 and FC.fp_class("v_subrev_f32_e32") == 2 and FC.fp_class("v_pk_add_f32") == 2
    for op in ("v_fma_f64", "v_fma_f16", "v_add_u32_e32", "v_mul_lo_u32", "v_mul_f32x", "s_mul_i32", "v_add_f32_foo"):
        assert FC.fp_class(op) is None, op


def test_triples_per_line(tmp_path):
    a = _write(tmp_path, "a.s", LISTING_A)
    assert FC.kernel_names(a) == ["_Z7kernelAv", "_Z7kernelBv"]
    assert FC.file_table(a) == {1: "dx_step.hip", 2: "dx_device.h"}
    ca = FC.census(a, "kernelA")
    assert ca == {("dx_device.h", 20): [1, 2, 1], ("dx_device.h", 21): [2, 0, 0], ("dx_step.hip", 30): [1, 1, 2]}
    assert FC.totals(ca) == (4, 3, 3)
    cb = FC.census(a, "kernelB")
    assert cb == {("dx_step.hip", 40): [0, 2, 2], ("dx_step.hip", 50): [1, 0, 0]}
    text = FC.format_census(ca)
    assert "dx_device.h:20  fused 1 mul 2 add 1" in text and text.endswith("total  fused 4 mul 3 add 3  (3 lines)")


def test_scaled():
    assert FC.scaled((1, 1, 2), (2, 2, 4)) and FC.scaled((0, 4, 2), (0, 2, 1))
    assert not FC.scaled((1, 1, 2), (1, 1, 2)) and not FC.scaled((1, 2, 1), (0, 3, 2))
    assert not FC.scaled((0, 0, 0), (1, 1, 1)) and not FC.scaled((1, 0, 0), (0, 1, 0))


def test_diff_and_marks(tmp_path):
    a, b = _write(tmp_path, "a.s", LISTING_A), _write(tmp_path, "b.s", LISTING_B)
    rows = FC.diff(FC.census(a, "kernelA"), FC.census(b, "kernelA"))
    assert rows == [("dx_device.h", 20, (1, 2, 1), (0, 3, 2), "FUSION"),
                    ("dx_step.hip", 30, (1, 1, 2), (2, 2, 4), "copies")]
    rows = FC.diff(FC.census(a, "kernelB"), FC.census(b, "kernelB"))
    assert rows == [("dx_step.hip", 40, (0, 2, 2), (0, 1, 1), "copies"),
                    ("dx_step.hip", 50, (1, 0, 0), (0, 0, 0), "only-a"),
                    ("dx_step.hip", 53, (0, 0, 0), (1, 0, 0), "only-b")]
    # three lines appeared in dx_step.hip at line 45 of the second listing
    lm = FC.parse_map(["dx_step.hip:+3@45"])
    assert lm == [("dx_step.hip", 3, 45)]
    rows = FC.diff(FC.census(a, "kernelB"), FC.census(b, "kernelB", lm))
    assert rows == [("dx_step.hip", 40, (0, 2, 2), (0, 1, 1), "copies")]
    text = FC.diff_listings(a, b)
    assert text.splitlines() == [
        "kernel _Z7kernelAv",
        "dx_device.h:20  1/2/1 -> 0/3/2  FUSION",
        "dx_step.hip:30  1/1/2 -> 2/2/4  copies",
        "2 lines differ, 1 other than copy-count changes",
        "totals fused/mul/add  4/3/3 -> 4/5/6",
        "kernel _Z7kernelBv",
        "dx_step.hip:40  0/2/2 -> 0/1/1  copies",
        "dx_step.hip:50  1/0/0 -> 0/0/0  only-a",
        "dx_step.hip:53  0/0/0 -> 1/0/0  only-b",
        "3 lines differ, 2 other than copy-count changes",
        "totals fused/mul/add  1/2/2 -> 1/1/1",
    ]
    assert FC.diff_listings(a, a, "kernelA").splitlines()[1] == "0 lines differ, 0 other than copy-count changes"


def test_instruction_stream_ignores_directives(tmp_path):
    a = _write(tmp_path, "a.s", LISTING_A)
    stripped = "\n".join(ln for ln in LISTING_A.splitlines() if not ln.strip().startswith((".loc", ".file")))
    b = _write(tmp_path, "b.s", stripped + "\n")
    sa = FC.instruction_stream(a)
    assert sa == FC.instruction_stream(b)
    assert "v_mul_f32_e32 v1, v0, v0" in sa and ".LBB0_1:" in sa and not any(s.startswith(".loc") for s in sa)
