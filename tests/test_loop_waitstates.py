"""The wait states hipcc adds around the inline assembly of the transform, counted on the CPU build (hipcc cross-compiles gfx950 without a GPU).

hipcc's hazard recogniser puts an `s_nop 0` in front of an inline-assembly statement that touches a register of the instruction directly
before it, and behind one of its own packed instructions whose result the next instruction reads.  A complex multiply written as two
statements (octfft::cmul) therefore costs three issue slots, and the persistent loop of the headline kernel is bound by instruction issue
(DESIGN.md 5.1).  The fused and the real-input kernels multiply two to a statement (octfft::cmul2 / cmul_const2, fft_pass PAIR): mul a,
mul b, fma a, fma b with the results out of place.  What is held here:

  * the `s_nop` count of the loops -- the headline loop had 26 and has 3 (one inside the statement of the product without a partner, two in
    front of add_i / sub_i statements); the bound is the 6 the change set out to reach;
  * the same work: the static VALU count of the headline loop and its packed multiplies / FMAs are what they were, registers too;
  * the rule the paired statements are built on: inside an assembly block no packed instruction directly follows the instruction that
    defines one of its sources, so nothing depends on whether the hardware forwards a packed FP32 result to the very next instruction.

The parent's counts were taken with this file's loop finder from a cross-compile of commit 2f839b0 ("N = 1024 fused kernel: straight-line
staging, mirror tap in line") with the flags csrc/Makefile gives each object: headline `<10,1,2,4>` 26, `<11,1,2,4>` 42 (48 in the whole
kernel), real-input `oct_real2_kernel<2,4>` 20.  Compiled as tests/test_headline_loop_valu.py does."""
import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
HEADLINE = "_ZN3oct16oct_fused_kernelILi10ELi1ELi2ELi4EEEvNS_9FusedArgsE"
N2048 = "_ZN3oct16oct_fused_kernelILi11ELi1ELi2ELi4EEEvNS_9FusedArgsE"
REAL2 = "_ZN3oct16oct_real2_kernelILi2ELi4EEEvNS_9FusedArgsE"
PARENT_S_NOP = {HEADLINE: 26, N2048: 42, REAL2: 20}
PARENT_HEADLINE_VALU, PARENT_HEADLINE_PK_MUL, PARENT_HEADLINE_PK_FMA, PARENT_HEADLINE_PK_ADD = 429, 53, 63, 140


def loop_of(lines, kernel):
    """(the lines of the kernel's largest backward branch -- the persistent loop --, the resource comment block behind the kernel)"""
    start = next(i for i, l in enumerate(lines) if l.startswith(kernel + ":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = lines[start:end]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    best = (0, 0, 0)
    for i, l in enumerate(body):
        m = re.search(r"s_(?:c)?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > best[0]:
            best = (i - labels[m.group(1)], labels[m.group(1)], i)
    loop = body[best[1]:best[2] + 1]
    assert len(loop) > 500, "the persistent loop was not found"
    return loop, "\n".join(lines[end:end + 400])


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """{kernel: (loop lines, resource block)} of the three kernels, from three cross-compiles run side by side"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("waitstates")
    ilp = re.search(r"^SCHED_ILP\s*:=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    base = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value", "-S", "--cuda-device-only"]
    units = {  # the flags of fused_10_rs2.o, fused_11_rs2.o and real2.o
        HEADLINE: (ilp + ["-DOCT_LOG2N=10", "-DOCT_FUSED_RS=2"], "fused_inst.hip"),
        N2048: (["-DOCT_LOG2N=11", "-DOCT_FUSED_RS=2"], "fused_inst.hip"),
        REAL2: (ilp, "real2_inst.hip"),
    }
    procs = {k: subprocess.Popen(base + flags + ["-o", str(tmp / ("%d.s" % i)), src], cwd=CSRC, stderr=subprocess.DEVNULL)
             for i, (k, (flags, src)) in enumerate(units.items())}
    out = {}
    for i, (k, pr) in enumerate(procs.items()):
        assert pr.wait() == 0, "hipcc failed on " + units[k][1]
        out[k] = loop_of(open(str(tmp / ("%d.s" % i))).read().split("\n"), k)
    return out


def instructions(loop):
    return [l.strip() for l in loop if l.strip() and not l.strip().startswith((";", "."))]


def opcodes(loop):
    return collections.Counter(l.split()[0] for l in instructions(loop))


def test_headline_loop_holds_at_most_six_wait_states(asm):
    ops = opcodes(asm[HEADLINE][0])
    print("s_nop in the headline loop: %d (parent: %d)" % (ops["s_nop"], PARENT_S_NOP[HEADLINE]))
    assert ops["s_nop"] <= 6


def test_headline_loop_does_the_same_work(asm):
    ops = opcodes(asm[HEADLINE][0])
    valu = sum(n for op, n in ops.items() if op.startswith("v_"))
    assert valu == PARENT_HEADLINE_VALU, "%d static VALU instructions in the loop" % valu
    packed = (ops["v_pk_mul_f32"], ops["v_pk_fma_f32"], ops["v_pk_add_f32"])
    assert packed == (PARENT_HEADLINE_PK_MUL, PARENT_HEADLINE_PK_FMA, PARENT_HEADLINE_PK_ADD), packed


def test_headline_register_budget(asm):
    meta = asm[HEADLINE][1]
    assert int(re.search(r"; NumVgprs: (\d+)", meta).group(1)) <= 256
    assert int(re.search(r"; ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"; Occupancy: (\d+)", meta).group(1)) >= 2


@pytest.mark.parametrize("kernel", [N2048, REAL2], ids=["n2048", "real_input"])
def test_other_loops_hold_no_more_wait_states_than_the_parent(asm, kernel):
    loop, meta = asm[kernel]
    n = opcodes(loop)["s_nop"]
    print("s_nop in the loop: %d (parent: %d)" % (n, PARENT_S_NOP[kernel]))
    assert n <= PARENT_S_NOP[kernel]
    assert int(re.search(r"; NumVgprs: (\d+)", meta).group(1)) <= 256
    assert int(re.search(r"; ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"; Occupancy: (\d+)", meta).group(1)) >= 2


# ---- the structural rule
def registers(operand):
    """the set of (file, index) an operand such as v[10:11], v3 or s[16:17] names"""
    m = re.match(r"^([vsa])\[(\d+):(\d+)\]$", operand)
    if m:
        return {(m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1)}
    m = re.match(r"^([vsa])(\d+)$", operand)
    return {(m.group(1), int(m.group(2)))} if m else set()


def operands(instruction):
    rest = instruction.split(None, 1)[1] if " " in instruction or "\t" in instruction else ""
    rest = re.split(r"\s+(?:op_sel|op_sel_hi|neg_lo|neg_hi|clamp|offset|offset0|offset1|offen|idxen|glc|nt|sc0|sc1)\b", rest)[0]
    return [o.strip() for o in rest.split(",") if o.strip()]


def defined(instruction):
    """the registers an instruction writes: its first operand, both operands of a lane swap, nothing for stores, waits and branches"""
    op = instruction.split()[0]
    if "store" in op or "write" in op or op.startswith(("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_barrier", "s_setprio", "s_endpgm")):
        return set()
    ops = operands(instruction)
    if not ops:
        return set()
    out = registers(ops[0])
    if "_swap" in op and len(ops) > 1:
        out |= registers(ops[1])
    return out


def unpadded_pairs(loop):
    """(producer, packed consumer) pairs where the consumer sits inside an assembly block directly behind the instruction that defines
    one of its sources, comment lines ignored"""
    bad, inside, prev = [], False, None
    for l in loop:
        s = l.strip()
        if "#ASMSTART" in s:
            inside = True
            continue
        if "#ASMEND" in s:
            inside = False
            continue
        if not s or s.startswith((";", ".")) or re.match(r"^\S+:$", s):
            continue
        if inside and s.startswith("v_pk_") and prev is not None:
            sources = set()
            for o in operands(s)[1:]:
                sources |= registers(o)
            if defined(prev) & sources:
                bad.append((prev, s))
        prev = s
    return bad


def test_the_rule_finds_what_it_is_for():
    mul = "v_pk_mul_f32 v[2:3], v[4:5], v[6:7] op_sel:[0,0] op_sel_hi:[0,1]"
    fma = "v_pk_fma_f32 v[2:3], v[4:5], v[6:7], v[2:3] op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"
    other = "v_pk_mul_f32 v[8:9], v[10:11], s[16:17] op_sel:[0,0] op_sel_hi:[0,1]"
    assert unpadded_pairs([";;#ASMSTART", mul, "; a comment", fma, ";;#ASMEND"]) == [(mul, fma)]
    assert unpadded_pairs([";;#ASMSTART", mul, "s_nop 0", fma, ";;#ASMEND"]) == []
    assert unpadded_pairs([";;#ASMSTART", mul, other, fma, ";;#ASMEND"]) == []
    assert unpadded_pairs(["v_permlane32_swap_b32_e32 v20, v5", ";;#ASMSTART", mul, ";;#ASMEND"]) == [("v_permlane32_swap_b32_e32 v20, v5", mul)]
    assert unpadded_pairs(["ds_read2_b64 v[4:7], v1 offset1:1", ";;#ASMSTART", mul, ";;#ASMEND"]) == [("ds_read2_b64 v[4:7], v1 offset1:1", mul)]
    assert unpadded_pairs(["s_mov_b32 s16, 0x3f800000", ";;#ASMSTART", other, ";;#ASMEND"]) == [("s_mov_b32 s16, 0x3f800000", other)]
    assert unpadded_pairs([mul, fma]) == [], "outside an assembly block the pair is hipcc's to pad"
    assert unpadded_pairs(["buffer_store_dword v4, v1, s[0:3], 0 offen nt", ";;#ASMSTART", mul, ";;#ASMEND"]) == []


@pytest.mark.parametrize("kernel", [HEADLINE, N2048, REAL2], ids=["headline", "n2048", "real_input"])
def test_no_packed_instruction_in_an_asm_block_directly_follows_the_definition_of_a_source(asm, kernel):
    loop = asm[kernel][0]
    assert sum(1 for l in loop if "#ASMSTART" in l) > 20, "the loop's assembly blocks were not found"
    bad = unpadded_pairs(loop)
    assert not bad, "\n".join("%s  ->  %s" % b for b in bad)
