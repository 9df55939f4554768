"""The instruction count of the headline kernel's persistent loop, checked on the CPU build (hipcc cross-compiles gfx950 without a GPU).

The loop of `oct_fused_kernel<10, IN_U16, RS_CUBIC, MODE_LOG>` is bound by vector-ALU issue, so instructions that are not
arithmetic on the signal -- format conversion by bit tricks, exchange addresses rebuilt per A-scan, rotations by i made of v_xor / v_mov --
cost time the image does not need.  They were taken out; a compiler update, or a change to the staging, the exchange or the
butterflies, can bring them back without any parity test noticing.  Compiled the way csrc/Makefile builds fused_10_rs2.o, as
tests/test_isa_shape.py does."""
import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNEL = "_ZN3oct16oct_fused_kernelILi10ELi1ELi2ELi4EEEvNS_9FusedArgsE"


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    """(opcode counts of the loop, the kernel's resource comment block)"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("valu") / "fused_10_rs2.s")
    flags = re.search(r"^SCHED_ILP\s*:=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value"] + flags +
                          ["-DOCT_LOG2N=10", "-DOCT_FUSED_RS=2", "-S", "--cuda-device-only", "-o", out, "fused_inst.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL + ":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = lines[start:end]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    best = (0, 0, 0)  # the largest backward branch: the persistent loop
    for i, l in enumerate(body):
        m = re.search(r"s_(?:c)?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > best[0]:
            best = (i - labels[m.group(1)], labels[m.group(1)], i)
    loop = [l.strip() for l in body[best[1]:best[2] + 1] if l.strip() and not l.strip().startswith((";", "."))]
    assert len(loop) > 500, "the persistent loop was not found"
    return collections.Counter(l.split()[0] for l in loop), "\n".join(lines[end:end + 400])


def test_loop_holds_at_most_440_vector_alu_instructions(kernel):
    ops, _ = kernel
    valu = sum(n for op, n in ops.items() if op.startswith("v_"))
    assert valu <= 440, "%d static VALU instructions in the loop (453 before the non-arithmetic ones were taken out): %s" % (
        valu, ", ".join("%d %s" % (n, op) for op, n in ops.most_common() if op.startswith("v_")))


def test_half_words_are_converted_by_one_instruction_each(kernel):
    ops, _ = kernel
    assert ops["v_perm_b32"] == 0, "the 2^23 bit trick (v_perm_b32 + packed subtract, 1.5 instructions per sample) is back"
    assert ops["v_cvt_f32_u32_sdwa"] == 16, "one half-word conversion per sample of the executed path"


def test_exchange_write_addresses_are_not_rebuilt_per_ascan(kernel):
    ops, _ = kernel
    # what is left: the four bases of the exchange READS (their span of 8 160 bytes exceeds the offset field of ds_read2_b64) and the
    # staging address -- hoisting either measured slower or spilled (tools/experiments/README.md).  13 before: 8 write bases on top.
    adds = sum(n for op, n in ops.items() if op.startswith("v_add_u32"))
    assert adds <= 5, "%d v_add_u32 in the loop" % adds
    assert ops["ds_write2_b64"] == 8, "the exchange writes are eight ds_write2_b64"
    # merged into 16-byte writes at 8-byte-aligned addresses the exchange runs at a seventh of the speed: the four of the staged row
    # (16-byte aligned) and the two of the `>> 4` path are all there may be
    assert ops["ds_write_b128"] <= 6, "%d ds_write_b128 in the loop" % ops["ds_write_b128"]


def test_rotations_by_i_are_operand_modifiers(kernel):
    ops, _ = kernel
    assert ops["v_xor_b32_e32"] == 0, "a sign flip as an instruction of its own: the rotation by i of the radix-16 passes is data movement again"
    assert ops["v_mov_b32_e32"] <= 2


def test_register_budget(kernel):
    _, meta = kernel
    assert int(re.search(r"; NumVgprs: (\d+)", meta).group(1)) <= 256
    assert int(re.search(r"; ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"; Occupancy: (\d+)", meta).group(1)) >= 2
