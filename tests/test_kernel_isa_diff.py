"""CPU: the classifier of tools/kernel_isa_diff.py, which decides whether a change to shared device code left a kernel's
generated code alone (identical), only moved register names (renamed) or changed the instruction stream (rescheduled)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_isa_diff as kid  # noqa: E402


def listing(body, vgpr=12):
    return (".globl demo_kernel\n"
            "demo_kernel:                            ; @demo_kernel\n"
            "; %bb.0:\n" + body +
            ".Lfunc_end3:\n"
            "\t.amdhsa_kernel demo_kernel\n"
            "\t\t.amdhsa_private_segment_fixed_size 0\n"
            f"\t\t.amdhsa_next_free_vgpr {vgpr}\n"
            "\t\t.amdhsa_next_free_sgpr 8\n"
            "\t.end_amdhsa_kernel\n")


BASE = ("\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n"
        "\tv_lshlrev_b32_e32 v2, 2, v0\n"
        ".LBB3_1:                                ; =>This Inner Loop Header: Depth=1\n"
        "\tv_add_f32_e32 v3, v2, v2\n"
        "\tv_mul_f32_e32 v4, v3, v2\n"
        "\tglobal_store_dword v2, v4, s[0:1] offset:16\n"
        "\ts_cbranch_scc1 .LBB3_1\n"
        "\ts_endpgm\n")


def one(text):
    return kid.kernels_text(text)["demo_kernel"]


def test_identical_ignores_comments_and_block_numbers():
    moved = BASE.replace("LBB3_", "LBB17_").replace("; =>This Inner Loop Header: Depth=1", "; other words")
    assert kid.classify(one(listing(BASE)), one(listing(moved))) == "identical"


def test_renamed_is_the_same_opcodes_in_the_same_order_with_the_same_descriptor():
    renamed = BASE.replace("v3", "v22").replace("v4", "v[20:21]").replace("offset:16", "offset:32")
    assert renamed != BASE
    assert kid.classify(one(listing(BASE)), one(listing(renamed))) == "renamed"
    # the same instruction stream with other resources is not a renaming
    assert kid.classify(one(listing(BASE, vgpr=12)), one(listing(renamed, vgpr=13))) == "rescheduled"


def test_rescheduled_is_any_other_order_or_instruction():
    lines = BASE.splitlines(keepends=True)
    lines[3], lines[4] = lines[4], lines[3]                # two instructions swapped
    assert kid.classify(one(listing(BASE)), one(listing("".join(lines)))) == "rescheduled"
    other = BASE.replace("v_mul_f32_e32 v4, v3, v2", "v_fma_f32 v4, v3, v2, v2")
    assert kid.classify(one(listing(BASE)), one(listing(other))) == "rescheduled"
    # a label that moves is a different schedule too
    lines = BASE.splitlines(keepends=True)
    lines[2], lines[3] = lines[3], lines[2]
    assert kid.classify(one(listing(BASE)), one(listing("".join(lines)))) == "rescheduled"
    assert kid.resources(one(listing(BASE, vgpr=40)))[:3] == ("40", "8", "0")
