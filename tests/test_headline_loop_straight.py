"""The control flow of the headline kernel's staging, checked on the CPU build (hipcc cross-compiles gfx950 without a GPU).

The persistent loop of `oct_fused_kernel<10, IN_U16, RS_CUBIC, MODE_LOG>` used to execute nine taken branches per A-scan where the
loop-back alone is needed: hipcc evaluated the `>> 4` test of chunk_to_float once per 256-sample chunk and reached every group of
SDWA conversions through a block behind the kernel's end, and the mirror tap of the cubic gather was an s_and_saveexec_b64 with
another such round trip.  The staging now tests the shift once per row (two straight-line arms, shared LDS writes) and the whole wave
writes the mirror tap in line: -1.5 to -2 % kernel time (profiles/headline_straight_items_ab.txt, headline_straight_final_ab.txt).
Where hipcc puts the arms hangs on a branch probability in the source and on the compiler's block placement; no parity test notices
when the out-of-line blocks come back.  Compiled the way csrc/Makefile builds fused_10_rs2.o, as tests/test_headline_loop_valu.py does.

(The planar pruned last pass with the packed epilogue measured 0.5 - 1.4 % SLOWER on this kernel and is not in the code --
tools/experiments/README.md -- so the loop keeps its eight v_add_f32, eight v_fma_f32 and the v_mov_b32 of the offset, and this file
holds no assertion on them.)"""
import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "octproz_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNEL = "_ZN3oct16oct_fused_kernelILi10ELi1ELi2ELi4EEEvNS_9FusedArgsE"
BRANCH = re.compile(r"^s_(?:c)?branch\S*\s+(\.LBB\d+_\d+)")


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    """(instructions and labels of the loop's span in order, labels inside the span, the kernel's resource comment block)"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("straight") / "fused_10_rs2.s")
    flags = re.search(r"^SCHED_ILP\s*:=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value"] + flags +
                          ["-DOCT_LOG2N=10", "-DOCT_FUSED_RS=2", "-S", "--cuda-device-only", "-o", out, "fused_inst.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL + ":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = lines[start:end]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    best = (0, 0, 0)  # the largest backward branch: the persistent loop, from its first label to the branch back
    for i, l in enumerate(body):
        m = re.search(r"s_(?:c)?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > best[0]:
            best = (i - labels[m.group(1)], labels[m.group(1)], i)
    span = [l.strip() for l in body[best[1]:best[2] + 1] if l.strip() and not l.strip().startswith(";")]
    span = [l for l in span if not l.startswith(".") or re.match(r"^\.LBB\d+_\d+:", l)]
    inside = {l.split(":")[0] for l in span if l.startswith(".LBB")}
    assert sum(1 for l in span if not l.startswith(".")) > 500, "the persistent loop was not found"
    return span, inside, "\n".join(lines[end:end + 400])


def staging(span):
    """from the loop header -- the label the loop is entered at, behind the tail of the previous A-scan's epilogue -- to the gather"""
    stores = [i for i, l in enumerate(span) if l.startswith("buffer_store_dword")]
    header = next(i for i in range(stores[-1], len(span)) if span[i].startswith(".LBB"))
    gather = next(i for i in range(header, len(span)) if span[i].startswith("s_setprio 3"))
    return span[header:gather]


def test_staging_holds_at_most_four_branches_and_none_leaves_the_loop(kernel):
    span, inside, _ = kernel
    br = [BRANCH.match(l) for l in staging(span)]
    br = [m for m in br if m]
    # the shift test, the skip of the no-shift arm behind the `>> 4` arm, the skip of the prefetch behind the wave's last row
    assert len(br) <= 4, "%d branch instructions in the staging: %s" % (len(br), [m.group(0) for m in br])
    out = [m.group(0) for m in br if m.group(1) not in inside]
    assert not out, "the staging branches to blocks outside the loop's span (11 branches and 5 such blocks before): %s" % out


def test_no_branch_of_the_loop_leaves_its_span_but_the_exit(kernel):
    span, inside, _ = kernel
    out = [l for l in span if BRANCH.match(l) and BRANCH.match(l).group(1) not in inside]
    assert len(out) <= 1, "blocks of the loop lie behind the kernel's end again: %s" % out


def test_both_arms_are_straight_line_and_share_the_row_writes(kernel):
    span, _, _ = kernel
    ops = collections.Counter(l.split()[0] for l in staging(span) if not l.startswith("."))
    assert ops["v_cvt_f32_u32_sdwa"] == 16 and ops["v_cvt_f32_u32_e32"] == 16, "one no-shift and one `>> 4` arm of sixteen conversions each: %s" % dict(ops)
    assert ops["ds_write_b128"] == 4, "the row writes are shared by the arms: %d ds_write_b128 in the staging" % ops["ds_write_b128"]
    # counted waits per chunk in both arms: the staging never waits for the stores issued a moment ago (tests/test_isa_shape.py holds the bound)
    waits = sorted(int(re.search(r"vmcnt\((\d+)\)", l).group(1)) for l in staging(span) if l.startswith("s_waitcnt") and "vmcnt" in l)
    assert waits == [8, 8, 9, 9, 10, 10, 11, 11], waits


def test_shift_flag_is_not_rebuilt_in_a_vector_register(kernel):
    span, _, _ = kernel
    ops = collections.Counter(l.split()[0] for l in span if not l.startswith("."))
    bad = {op: n for op, n in ops.items() if op.startswith("v_cndmask_b32") or op.startswith("v_cmp")}
    assert not bad, "the loop rebuilds a flag through the vector ALU per A-scan: %s" % bad


def test_mirror_tap_is_one_lds_write_of_the_whole_wave(kernel):
    span, _, _ = kernel
    st = staging(span)
    ops = collections.Counter(l.split()[0] for l in st if not l.startswith("."))
    assert ops["ds_write_b32"] == 1, "%d ds_write_b32 in the staging" % ops["ds_write_b32"]
    assert not any("exec" in l for l in st if not l.startswith("s_and_b64 vcc") and not l.startswith("s_andn2_b64 vcc")), \
        "the staging changes the exec mask: %s" % [l for l in st if "exec" in l]
    # ... in front of the row write that overwrites what the lanes other than 0 wrote
    first = next(i for i, l in enumerate(st) if l.startswith("ds_write_b"))
    assert st[first].startswith("ds_write_b32"), st[first]


def test_budgets(kernel):
    span, _, meta = kernel
    valu = sum(1 for l in span if l.startswith("v_"))
    # 432 before; both arms of the shift are in the span (32 instructions of the `>> 4` arm do not execute with the benchmark's settings)
    assert valu <= 429, "%d static VALU instructions in the loop" % valu
    assert int(re.search(r"; NumVgprs: (\d+)", meta).group(1)) <= 256
    assert int(re.search(r"; ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"; Occupancy: (\d+)", meta).group(1)) == 2
