"""Static wait-state check of the hand-written inline asm in the shipped kernels.

LLVM's hazard recogniser pads the compiler's own instruction pairs with `s_nop`, but it does not look inside an `asm(...)` string: a pair
whose producer or consumer was written by hand gets no padding, and a missing wait state shows up as wrong values on some waves of some
launches, with no fault (tgs_device.hpp, HAZARDS).  This module compiles the library's sources to gfx950 assembly with the build's own
flags, walks every function's instruction stream (across labels, into every predecessor block) and reports each pair from RULES whose
producer or consumer lies between `;;#ASMSTART` and `;;#ASMEND` and that has fewer wait states between them than the rule asks for.

Wait states are counted the way the hardware counts them: 1 per instruction, N + 1 for `s_nop N`; labels, directives and comments are 0.
Like LLVM, the walk looks for the nearest hazardous producers and does not stop at a non-hazardous write of the same register in between.

  python -m tests.isa_hazards [-DNAME=VALUE ...]      prints every violation of the library as it stands
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- instructions and their registers -------------------------------------------------------------------------------------------

@dataclass
class Ins:
    text: str                  # the instruction as printed (comment stripped)
    op: str                    # mnemonic
    ops: list                  # operand tokens, modifiers dropped
    asm: bool                  # between ;;#ASMSTART and ;;#ASMEND
    line: int                  # 1-based line in the .s (0 for snippets built by hand)

    @property
    def waits(self) -> int:
        if self.op == "s_nop":
            return int(self.ops[0], 0) + 1 if self.ops else 1
        return 1

    @property
    def valu(self) -> bool:
        return self.op.startswith("v_")


_RANGE = re.compile(r"^([vsa])\[(\d+):(\d+)\]$")
_SINGLE = re.compile(r"^([vsa])(\d+)$")


def regs(tok: str) -> frozenset:
    """the 32-bit registers an operand names: v5 -> {v5}, s[4:5] -> {s4, s5}, vcc -> {vcc_lo, vcc_hi}; constants and the like -> {}"""
    t = tok.strip().lstrip("-|")
    for pre in ("abs(", "neg(", "sext("):
        if t.startswith(pre):
            t = t[len(pre):]
    t = t.rstrip("|)")
    m = _SINGLE.match(t)
    if m:
        return frozenset([t])
    m = _RANGE.match(t)
    if m:
        return frozenset(f"{m.group(1)}{i}" for i in range(int(m.group(2)), int(m.group(3)) + 1))
    if t in ("vcc", "exec"):
        return frozenset([t + "_lo", t + "_hi"])
    if t in ("vcc_lo", "vcc_hi", "exec_lo", "exec_hi", "m0"):
        return frozenset([t])
    return frozenset()


def _split_operands(rest: str) -> list:
    """top-level comma split (quad_perm:[1,0,3,2] keeps its commas); each operand's first word (modifiers follow the last one)"""
    out, depth, cur = [], 0, ""
    for ch in rest:
        if ch in "[(":
            depth += 1
        elif ch in "])":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    toks = []
    for o in out:
        o = o.strip()
        # a word is split off at a space outside brackets ("v2 quad_perm:[1, 0, 3, 2] row_mask:0xf" -> "v2")
        depth, end = 0, len(o)
        for i, ch in enumerate(o):
            if ch in "[(":
                depth += 1
            elif ch in "])":
                depth -= 1
            elif ch.isspace() and depth == 0:
                end = i
                break
        toks.append(o[:end])
    return toks


def parse_ins(text: str, asm: bool = False, line: int = 0) -> Ins:
    text = text.split(";")[0].strip()
    parts = text.split(None, 1)
    return Ins(text, parts[0], _split_operands(parts[1]) if len(parts) > 1 else [], asm, line)


_CARRY_OUT = re.compile(r"^v_(add|sub|subrev|addc|subb|subbrev)_co_u32|^v_div_scale_f(32|64)|^v_mad_(u64_u32|i64_i32)")
_TRANS = re.compile(r"^v_(exp|log|rcp|rsq|sqrt|sin|cos)(_legacy|_iflag|_clamp)?_f(16|32|64)")


def _is_permlane_swap(i: Ins) -> bool:
    return i.op.startswith("v_permlane") and i.op.endswith("_swap_b32")


def valu_defs(i: Ins) -> frozenset:
    """registers a VALU instruction writes"""
    if not i.valu or i.op == "v_nop" or not i.ops:
        return frozenset()
    d = set(regs(i.ops[0]))
    if _is_permlane_swap(i):
        d |= regs(i.ops[1])
    elif i.op.startswith("v_cmpx"):
        d |= regs("exec")
    elif _CARRY_OUT.match(i.op) and len(i.ops) > 1:
        d |= regs(i.ops[1])
    return frozenset(d)


def valu_uses(i: Ins) -> frozenset:
    """registers a VALU instruction reads as operands (EXEC, read by every one of them, is not listed)"""
    if not i.valu or i.op == "v_nop":
        return frozenset()
    if _is_permlane_swap(i):
        return frozenset(r for o in i.ops for r in regs(o))
    first = 2 if _CARRY_OUT.match(i.op) else 1
    u = set(r for o in i.ops[first:] for r in regs(o))
    if i.op.startswith("v_div_fmas"):
        u |= regs("vcc")
    return frozenset(u)


def _sgpr(r: str) -> bool:
    return (r[0] == "s" and r[1:].isdigit()) or r.startswith("vcc")


def _vgpr(r: str) -> bool:
    return r[0] == "v" and r[1:].isdigit()


# ---- the rule table -------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Rule:
    name: str
    need: int                  # wait states between producer and consumer
    prod: object               # Ins -> registers it writes as a hazardous producer
    cons: object               # Ins -> registers it reads as a hazardous consumer
    cite: str = ""             # source of a rule for which the compiler's own code gives no witness (test_isa_hazards checks)


def _is_dpp(i: Ins) -> bool:
    return i.op.endswith("_dpp")


RULES = (
    # v_cmp* to an SGPR pair or VCC, v_readlane / v_readfirstlane, carry-out -> a VALU reading that SGPR as an operand or a mask
    Rule("valu-write-sgpr -> valu-read", 2,
         lambda i: frozenset(r for r in valu_defs(i) if _sgpr(r)),
         lambda i: frozenset(r for r in valu_uses(i) if _sgpr(r))),
    # a VGPR written by a VALU -> a DPP instruction reading it
    Rule("valu-write-vgpr -> dpp-read", 2,
         lambda i: frozenset(r for r in valu_defs(i) if _vgpr(r)),
         lambda i: frozenset(r for r in valu_uses(i) if _vgpr(r)) if _is_dpp(i) else frozenset()),
    # a VGPR written by a VALU -> v_permlane{16,32}_swap reading it (gfx950)
    Rule("valu-write-vgpr -> permlane-swap-read", 2,
         lambda i: frozenset(r for r in valu_defs(i) if _vgpr(r)),
         lambda i: valu_uses(i) if _is_permlane_swap(i) else frozenset(),
         cite="cdna_hip_programming.md section 5.5 T21 (LLVM's gfx950 rule 'VALU write vdst -> v_permlane read': 2 wait states); "
              "the library's swaps are inline asm only, so the compiler emits no pair of its own"),
    # EXEC written by a VALU (v_cmpx) -> any DPP instruction
    Rule("valu-write-exec -> dpp", 5,
         lambda i: frozenset(r for r in valu_defs(i) if r.startswith("exec")),
         lambda i: regs("exec") if _is_dpp(i) else frozenset(),
         cite="CDNA3 / CDNA4 ISA reference, 'Manually Inserted Wait States': VALU writes EXEC -> VALU DPP op, 5 wait states "
              "(LLVM GCNHazardRecognizer::checkDPPHazards); the compiler writes EXEC with the scalar unit here, so it emits no such pair"),
    # a transcendental (v_exp, v_rcp, ...) result -> a VALU reading it (gfx940 family)
    Rule("trans-write-vgpr -> valu-read", 1,
         lambda i: frozenset(r for r in valu_defs(i) if _vgpr(r)) if _TRANS.match(i.op) else frozenset(),
         lambda i: frozenset(r for r in valu_uses(i) if _vgpr(r))),
    # a VGPR written by a VALU -> v_readlane / v_readfirstlane reading it as the source (gfx940 family)
    Rule("valu-write-vgpr -> readlane-src", 1,
         lambda i: frozenset(r for r in valu_defs(i) if _vgpr(r)),
         lambda i: regs(i.ops[1]) if i.op.startswith(("v_readlane", "v_readfirstlane")) and len(i.ops) > 1 else frozenset()),
)


# ---- functions, blocks and the walk ---------------------------------------------------------------------------------------------

@dataclass
class Block:
    label: str
    ins: list = field(default_factory=list)
    preds: list = field(default_factory=list)


_LABEL = re.compile(r"^([.\w$]+):")
_BRANCH = re.compile(r"^s_(c?branch\w*)$")


def blocks_of(lines) -> list:
    """basic blocks of one function body (lines as printed); a block ends at a label or behind a branch"""
    blocks = [Block("<entry>")]
    asm = False
    for ln, raw in lines:
        s = raw.strip()
        if s.startswith(";;#ASMSTART"):
            asm = True
            continue
        if s.startswith(";;#ASMEND"):
            asm = False
            continue
        if not s or s.startswith(";") or s.startswith("//"):
            continue
        m = _LABEL.match(s)
        if m:
            blocks.append(Block(m.group(1)))
            continue
        if s.startswith("."):
            continue                                              # directive
        i = parse_ins(s, asm, ln)
        blocks[-1].ins.append(i)
        if _BRANCH.match(i.op) or i.op in ("s_endpgm", "s_setpc_b64"):
            blocks.append(Block(""))                              # (unlabelled: reached by fall-through only)
    by_label = {b.label: k for k, b in enumerate(blocks) if b.label}
    for k, b in enumerate(blocks):
        last = b.ins[-1] if b.ins else None
        if last is not None and _BRANCH.match(last.op) and last.ops and last.ops[0] in by_label:
            blocks[by_label[last.ops[0]]].preds.append(k)
        ends = last is not None and (last.op in ("s_branch", "s_endpgm", "s_setpc_b64"))
        if not ends and k + 1 < len(blocks):
            blocks[k + 1].preds.append(k)
    return blocks


@dataclass
class Pair:
    rule: Rule
    prod: Ins
    cons: Ins
    waits: int                 # wait states between them (on the shortest path found)
    padded: bool               # an s_nop lies between them on that path


def pairs(blocks, rules=RULES):
    """every (producer, consumer) pair of every rule with at most rule.need wait states between them, on any path"""
    out = []
    for bk, b in enumerate(blocks):
        for ci, c in enumerate(b.ins):
            for rule in rules:
                want = rule.cons(c)
                if not want:
                    continue
                seen = set()
                stack = [(bk, ci, 0, False)]                     # (block, index of the instruction behind the next one to look at, waits, nop seen)
                while stack:
                    k, j, w, nop = stack.pop()
                    if (k, j, w, nop) in seen:
                        continue
                    seen.add((k, j, w, nop))
                    if j == 0:
                        for p in blocks[k].preds:
                            stack.append((p, len(blocks[p].ins), w, nop))
                        continue
                    p = blocks[k].ins[j - 1]
                    if rule.prod(p) & want:
                        out.append(Pair(rule, p, c, w, nop))
                    w2 = w + p.waits
                    if w2 <= rule.need:
                        stack.append((k, j - 1, w2, nop or p.op == "s_nop"))
    return out


def violations(blocks, rules=RULES, asm_only=True):
    """pairs with too few wait states; asm_only: producer or consumer is inline asm, else: neither is (the compiler's own pairs)"""
    return [p for p in pairs(blocks, rules) if p.waits < p.rule.need and (p.prod.asm or p.cons.asm) == asm_only]


# ---- the shipped code -----------------------------------------------------------------------------------------------------------

def functions_of(s_text: str) -> dict:
    """{mangled name: [(line number, line)]} of every function in a .s file"""
    lines = s_text.split("\n")
    names = set(re.findall(r"^\s*\.type\s+([\w.$]+),@function", s_text, re.M))
    funcs, cur = {}, None
    for n, l in enumerate(lines, 1):
        m = _LABEL.match(l)
        if m and m.group(1) in names:
            cur = m.group(1)
            funcs[cur] = []
            continue
        if cur is not None:
            if l.startswith(".Lfunc_end"):
                cur = None
                continue
            funcs[cur].append((n, l))
    return funcs


def demangle(names) -> dict:
    names = list(names)
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, timeout=60)
        out = r.stdout.split("\n")
        if r.returncode == 0 and len(out) >= len(names):
            return dict(zip(names, out))
    except (OSError, subprocess.SubprocessError):
        pass
    return {n: n for n in names}


def compile_sources(outdir: str, defines=()) -> dict:
    """{source: path of its gfx950 .s}: every source the library is built from, with the build's own flags (the code that ships)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from youreditableavatar_amd import build
    cc = build.hipcc()

    def one(src):
        out = os.path.join(outdir, src + ".s")
        cmd = [cc, *build.FLAGS, *build.EXTRA_FLAGS.get(src, []), *defines, "-S", "--cuda-device-only", os.path.join(build.CSRC, src), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc -S failed on {src}:\n{r.stderr}")
        return src, out

    with ThreadPoolExecutor(max_workers=min(len(build.SOURCES), 8)) as ex:
        return dict(ex.map(one, build.SOURCES))


@dataclass
class Unit:
    src: str
    name: str                  # demangled
    blocks: list


def load_units(s_files: dict) -> list:
    units = []
    for src, path in sorted(s_files.items()):
        funcs = functions_of(open(path).read())
        dm = demangle(funcs)
        units += [Unit(src, dm[n], blocks_of(body)) for n, body in funcs.items()]
    return units


def describe(unit: Unit, p: Pair) -> str:
    return (f"{unit.src}: {unit.name}: [{p.rule.name}] {p.prod.text!r} (line {p.prod.line}{', asm' if p.prod.asm else ''}) -> "
            f"{p.cons.text!r} (line {p.cons.line}{', asm' if p.cons.asm else ''}): {p.waits} wait state(s), {p.rule.need} needed")


def main(argv) -> int:
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        units = load_units(compile_sources(d, argv))
    bad = [describe(u, p) for u in units for p in violations(u.blocks)]
    print("\n".join(bad) if bad else "no inline-asm wait-state violations")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
