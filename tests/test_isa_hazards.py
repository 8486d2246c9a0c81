"""Wait states of the hand-written inline asm in the code that ships (tests/isa_hazards.py): CPU only, hipcc cross-compiles every source
of the library to gfx950 assembly with the build's own flags.  The rule table is calibrated on the compiler's own pairs: LLVM pads those,
so none of them may break a rule (the table is not stricter than LLVM's), and each rule the compiler meets itself must have a pair padded
to exactly its count (not laxer); a rule the compiler never meets cites where it comes from instead."""
import pytest

from tests import isa_hazards as H

# the library as built, and the A/B partner of the asm list appends (tgs_device.hpp, HAZARDS: -DTGS_QL_APPEND_C=1)
VARIANTS = {"default": (), "ql_append_c": ("-DTGS_QL_APPEND_C=1",)}


@pytest.fixture(scope="module", params=sorted(VARIANTS))
def shipped(request, tmp_path_factory):
    from youreditableavatar_amd import build
    try:
        build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp(f"isa_{request.param}")
    return H.load_units(H.compile_sources(str(d), VARIANTS[request.param]))


def test_every_source_and_kernel_is_read(shipped):
    from youreditableavatar_amd import build
    assert {u.src for u in shipped} >= set(build.SOURCES) - {"tgs_api.hip"}          # (tgs_api.hip is host code: no device function)
    names = {u.name.split("(")[0] for u in shipped}
    assert {"tgs::k_render_bwd", "tgs::k_render_fwd"} <= names, sorted(names)
    assert sum(len(b.ins) for u in shipped for b in u.blocks) > 10000
    assert sum(i.asm for u in shipped for b in u.blocks for i in b.ins) > 100


def test_inline_asm_has_its_wait_states(shipped):
    bad = [H.describe(u, p) for u in shipped for p in H.violations(u.blocks)]
    assert not bad, "inline asm too close to the instruction it depends on:\n" + "\n".join(bad)


def test_rule_table_is_not_stricter_than_llvm(shipped):
    bad = [H.describe(u, p) for u in shipped for p in H.violations(u.blocks, asm_only=False)]
    assert not bad, "the compiler's own pairs break the rule table:\n" + "\n".join(bad)


def test_rule_table_is_not_laxer_than_llvm(shipped):
    witnessed = {p.rule.name for u in shipped for p in H.pairs(u.blocks)
                 if not p.prod.asm and not p.cons.asm and p.padded and p.waits == p.rule.need}
    for r in H.RULES:
        assert r.name in witnessed or r.cite, f"{r.name}: no compiler pair padded to {r.need} wait state(s), and no citation"


# ---- the checker on snippets --------------------------------------------------------------------------------------------------------

def _check(text):
    return H.violations(H.blocks_of(list(enumerate(text.strip().split("\n"), 1))))


def _one(text, rule, waits):
    v = _check(text)
    assert [(p.rule.name, p.waits) for p in v] == [(rule, waits)], [(p.rule.name, p.prod.text, p.cons.text, p.waits) for p in v]


# what hipcc emitted for select_loaded at five places of k_render_bwd until the mask was formed on the scalar unit
SELECT_LOADED = """
    v_cmp_ne_u32_e64 s[8:9], 0, v3
    s_waitcnt vmcnt(7)
    ;;#ASMSTART
    v_cndmask_b32_e64 v8, 0, v9, s[8:9]
    ;;#ASMEND
"""


def test_select_loaded_sequence_is_flagged():
    _one(SELECT_LOADED, "valu-write-sgpr -> valu-read", 1)
    assert not _check(SELECT_LOADED.replace("s_waitcnt vmcnt(7)", "s_waitcnt vmcnt(7)\n    s_nop 0"))


def test_scalar_unit_mask_is_not_flagged():
    assert not _check("""
    v_cmp_ne_u32_e64 s[8:9], 0, v3
    ;;#ASMSTART
    s_and_b64 s[54:55], s[8:9], exec
    ;;#ASMEND
    ;;#ASMSTART
    v_cndmask_b32_e64 v8, 0, v9, s[54:55]
    ;;#ASMEND
""")


def test_s_nop_counts_n_plus_one():
    text = """
    v_add_f32_e32 v1, v2, v3
    s_nop {n}
    ;;#ASMSTART
    v_mov_b32_dpp v4, v1 quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf
    ;;#ASMEND
"""
    assert not _check(text.format(n=1))
    _one(text.format(n=0), "valu-write-vgpr -> dpp-read", 1)


@pytest.mark.parametrize("between", [0, 1])
def test_dpp_read_right_behind_its_write_is_flagged(between):
    _one("""
    ;;#ASMSTART
    v_sub_f32 v5, 1.0, v2
""" + "    v_mul_f32 v6, v2, v3\n" * between + """
    v_cndmask_b32_dpp v7, v5, v8, vcc quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf
    ;;#ASMEND
""", "valu-write-vgpr -> dpp-read", between)


QL_APPEND = """
    ;;#ASMSTART
    v_and_b32 v4, 0x400, v2
    v_cmp_ne_u32 vcc, 0, v4
    s_and_saveexec_b64 s[6:7], vcc
    s_bcnt1_i32_b64 s8, vcc
    v_mbcnt_lo_u32_b32 v5, vcc_lo, 0
    v_mbcnt_hi_u32_b32 v5, vcc_hi, v5
    v_lshl_add_u32 v5, v5, 1, s9
    ds_write_b16 v5, v3
    s_mov_b64 exec, s[6:7]
    ;;#ASMEND
"""


def test_ql_append_as_written_passes_and_without_s_bcnt1_is_flagged():
    assert not _check(QL_APPEND)
    _one(QL_APPEND.replace("    s_bcnt1_i32_b64 s8, vcc\n", ""), "valu-write-sgpr -> valu-read", 1)


def test_hazard_through_a_branch_to_a_label_is_flagged():
    text = """
    v_cmp_ne_u32_e64 s[8:9], 0, v3
    s_cbranch_execz .LBB0_2
    s_nop 7
    s_branch .LBB0_3
.LBB0_2:                                ; %pad
    ;;#ASMSTART
    v_cndmask_b32_e64 v8, 0, v9, s[8:9]
    ;;#ASMEND
.LBB0_3:
    s_endpgm
"""
    _one(text, "valu-write-sgpr -> valu-read", 1)
    assert not _check(text.replace("s_cbranch_execz", "s_nop 0\n    s_cbranch_execz"))


def test_fall_through_into_a_label_is_walked_and_an_unconditional_branch_is_not():
    fall = """
    v_rcp_f32_e32 v1, v2
.LBB0_1:
    ;;#ASMSTART
    v_mul_f32 v3, v1, v4
    ;;#ASMEND
    s_endpgm
"""
    _one(fall, "trans-write-vgpr -> valu-read", 0)
    assert not _check(fall.replace(".LBB0_1:", "s_branch .LBB0_2\n.LBB0_1:"))


def test_asm_producer_and_compiler_consumer_is_flagged():
    _one("""
    ;;#ASMSTART
    v_cmp_gt_i32 vcc, v1, v2
    ;;#ASMEND
    v_cndmask_b32_e32 v3, 0, v4, vcc
""", "valu-write-sgpr -> valu-read", 0)


def test_compiler_only_pairs_are_not_reported_as_asm_violations():
    text = SELECT_LOADED.replace(";;#ASMSTART", "").replace(";;#ASMEND", "")
    assert not _check(text)
    assert len(H.violations(H.blocks_of(list(enumerate(text.split("\n"), 1))), asm_only=False)) == 1


@pytest.mark.parametrize("swap", ["v_permlane32_swap_b32", "v_permlane16_swap_b32"])
def test_permlane_swap_needs_two(swap):
    text = f"""
    v_add_f32_e32 v2, v6, v7
    ;;#ASMSTART
    s_nop 1
    {swap} v1, v2
    ;;#ASMEND
"""
    assert not _check(text)
    _one(text.replace("s_nop 1", "s_nop 0"), "valu-write-vgpr -> permlane-swap-read", 1)


def test_valu_exec_write_before_dpp_needs_five():
    text = """
    v_cmpx_ne_u32_e64 s[0:1], 0, v3
    s_nop 3
    ;;#ASMSTART
    v_add_f32_dpp v1, v1, v2 row_ror:4 row_mask:0xf bank_mask:0xf
    ;;#ASMEND
"""
    assert not _check(text.replace("s_nop 3", "s_nop 4"))
    _one(text, "valu-write-exec -> dpp", 4)


def test_operands_and_registers():
    assert H.regs("s[8:9]") == {"s8", "s9"} and H.regs("v[4:7]") == {"v4", "v5", "v6", "v7"}
    assert H.regs("vcc") == {"vcc_lo", "vcc_hi"} and H.regs("-|v3|") == {"v3"} and H.regs("0x3c00") == set()
    i = H.parse_ins("v_cndmask_b32_dpp v7, v5, v8, vcc quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf")
    assert i.ops == ["v7", "v5", "v8", "vcc"]
    assert H.valu_defs(i) == {"v7"} and H.valu_uses(i) == {"v5", "v8", "vcc_lo", "vcc_hi"}
    c = H.parse_ins("v_addc_co_u32_e32 v1, vcc, v2, v3, vcc")
    assert H.valu_defs(c) == {"v1", "vcc_lo", "vcc_hi"} and H.valu_uses(c) == {"v2", "v3", "vcc_lo", "vcc_hi"}
    assert H.parse_ins("s_nop 4").waits == 5 and H.parse_ins("s_waitcnt vmcnt(7)").waits == 1
