"""Edges of the persistent loop of the N = 1024 uint16 kernels that a parity run on the benchmark data does not reach.

The loop converts the raw half-words with one `v_cvt_f32_u32` per sample that selects its half of the dword, and writes the first pass'
outputs from one base register, computed once per wave, with immediate offsets.  What can go wrong there shows (a) at the edges of a
half-word -- upper half, bit 15, the `>> 4` path that converts differently -- and (b) in the SECOND iteration of a wave, which runs
on the hoisted address and on a row prefetched during the first.  Every A-scan of every buffer is compared against the oracle with
the tolerances of tests/common.py, strict (no bin excused)."""
import numpy as np
import pytest

import common
from octproz_amd import Pipeline, _lib, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

N = 1024
EDGES = (0, 1, 4095, 32767, 32768, 65535)


def to_device(raw):
    import torch
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.int16)).to("cuda:0")


def raw16(A, B, seed):
    """the benchmark's synthetic fringes moved up to 16 bits with random low bits: every bit of a half-word is in use"""
    rng = np.random.default_rng(seed)
    r = synthetic_raw(N, A, B, seed=seed).astype(np.uint32).reshape(-1, N)
    return (r * 16 + rng.integers(0, 16, size=r.shape, dtype=np.uint32)).astype(np.uint16)


def with_edges(raw):
    """all 36 (lower half, upper half) pairs of EDGES in 36 dwords of every A-scan, spread over the four chunks of a row"""
    raw = raw.copy()
    k = 0
    for lo in EDGES:
        for hi in EDGES:
            d = 3 + 14 * k          # dword 3, 17, ... 493: both parities of the lane's two dwords, every 256-sample chunk
            raw[:, 2 * d], raw[:, 2 * d + 1] = lo, hi
            k += 1
    return raw


def run(p, raw, what, path=0):
    p.update_all_curves()
    o = common.make_oracle(p)
    want = o.process(raw)
    pipe = Pipeline(p, device=0)
    if p.fixedPatternNoiseRemoval:
        pipe.set_mean_line(o.mean_line(), pin=True)
    d = to_device(raw)
    pipe.process_device(d.data_ptr())
    pipe.synchronize()
    got = pipe.processed_host()
    assert pipe.last_path() & path == path, hex(pipe.last_path())
    grid = pipe.last_grid()
    common.compare_images(got, want, p, what, strict=True, mean_line=o.mean_line())
    pipe.close(); o.close()
    return grid


@pytest.mark.parametrize("bitshift", [0, 1])
@pytest.mark.parametrize("lines", [1, 7, 64])
def test_half_word_edges(lines, bitshift):
    p = v180_benchmark_params(N, lines, 1)
    p.bitDepth, p.bitshift = 16, bitshift
    if lines < 18:
        p.fixedPatternNoiseRemoval = 0  # fewer than 18 lines cannot give a mean line
    run(p, with_edges(raw16(lines, 1, seed=100 + lines)), "half-word edges, %d lines, bitshift %d" % (lines, bitshift))


def split(lines):
    """(A-scans per B-scan, B-scans) with the fewest B-scans >= 2 (the flip mirrors even B-scans that have a successor)"""
    for b in range(2, 65):
        if lines % b == 0:
            return lines // b, b
    return lines, 1


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("which", ["waves_plus_1", "three_rounds_minus_5"])
def test_loop_carried_addresses(which, flip):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = 8 * cus  # one workgroup of eight waves per CU (two waves per SIMD)
    lines = waves + 1 if which == "waves_plus_1" else 3 * (waves + 1) - 5
    A, B = split(lines)
    p = v180_benchmark_params(N, A, B)
    p.bscanFlip = flip
    grid = run(p, raw16(A, B, seed=7 + flip), "%s (%d lines as %d x %d), flip %d" % (which, lines, A, B, flip))
    assert grid == cus, "the grid is not one workgroup per CU (%d blocks, %d CUs): the buffer sizes of this test assume it" % (grid, cus)


def test_rolling_average_variant_on_the_edges():
    p = v180_benchmark_params(N, 64, 1)
    p.bitDepth, p.backgroundRemoval, p.rollingAverageWindowSize = 16, 1, 64
    run(p, with_edges(raw16(64, 1, seed=164)), "rolling average W = 64 on the half-word edges", _lib.PATH_ROLL_IN_KERNEL)


def test_real_input_route_on_the_edges():
    p = v180_benchmark_params(N, 64, 1)
    p.bitDepth, p.dispersionCompensation = 16, 0
    run(p, with_edges(raw16(64, 1, seed=264)), "real-input route on the half-word edges", _lib.PATH_REAL_INPUT)
