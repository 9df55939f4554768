"""The straight-line staging of the uint16 fused kernels against the oracle, where a parity run on the benchmark data does not look.

The persistent loop tests the `>> 4` shift once per row and converts the whole row in one of two straight-line arms; the mirror tap of
the cubic gather (sample -1 := sample 1) is written by the WHOLE wave in front of the row -- lane 0 hits sample -1, every other lane a
word of its neighbour's unit that the row write behind it overwrites.  What can go wrong there: an arm that converts differently, the
wave's last row (no prefetch behind it), a mirror tap that is missing, wrong or that survives in a neighbour's sample, the second
iteration of a wave, and every kernel variant that shares the staging.  Every A-scan of every buffer is compared against the oracle
with the tolerances of tests/common.py, strict (no bin excused), with the mean line pinned -- the harness of
tests/test_gpu_headline_loop_edges.py."""
import numpy as np
import pytest

import common
from octproz_amd import Pipeline, _lib, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

N = 1024


def to_device(raw):
    import torch
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.int16)).to("cuda:0")


def raw16(n, A, B, seed):
    """the benchmark's synthetic fringes moved up to 16 bits with random low bits: every bit of a half-word is in use"""
    rng = np.random.default_rng(seed)
    r = synthetic_raw(n, A, B, seed=seed).astype(np.uint32).reshape(-1, n)
    return (r * 16 + rng.integers(0, 16, size=r.shape, dtype=np.uint32)).astype(np.uint16)


def run(p, raw, what, path=0, route=0, clamped=False):
    p.update_all_curves()
    o = common.make_oracle(p)
    want = o.process(raw)
    pipe = Pipeline(p, device=0, route=route)
    if p.fixedPatternNoiseRemoval:
        pipe.set_mean_line(o.mean_line(), pin=True)
    d = to_device(raw)
    pipe.process_device(d.data_ptr())
    pipe.synchronize()
    got = pipe.processed_host()
    assert pipe.last_path() & path == path, hex(pipe.last_path())
    grid = pipe.last_grid()
    if clamped:
        # behind the clamp of the background removal the grey values are compared directly (both sides clamp the same way), with the
        # bound tests/test_gpu_parity.py holds this store to
        print("%s: max grey-value error %.3e" % (what, float(np.abs(got - want).max())))
        assert np.abs(got - want).max() < 1e-3, what
        assert got.min() >= 0.0 and got.max() <= 1.0, what
    else:
        rel, db = common.compare_images(got, want, p, what, strict=True, mean_line=o.mean_line())
        print("%s: max linear-power error %.2e, max normalised-dB error %.2e" % (what, rel, db))
    pipe.close(); o.close()
    return grid


@pytest.mark.parametrize("bitshift", [0, 1])
@pytest.mark.parametrize("lines", [1, 7, 64])
def test_both_arms_of_the_shift(lines, bitshift):
    """one row (no prefetch at all), seven (the wave's only row is its last) and 64"""
    p = v180_benchmark_params(N, lines, 1)
    p.bitDepth, p.bitshift = 16, bitshift
    if lines < 18:
        p.fixedPatternNoiseRemoval = 0  # fewer than 18 lines cannot give a mean line
    run(p, raw16(N, lines, 1, seed=300 + lines), "shift arms, %d lines, bitshift %d" % (lines, bitshift))


@pytest.mark.parametrize("bitshift", [0, 1])
def test_mirror_tap_feeds_the_first_bins(bitshift):
    """The benchmark's curve starts below sample 1 (c0 = 0.535), so the first output samples read tap -1.  Sample 1 of every row is the
    largest value and its neighbours are 0: a missing or wrong mirror tap changes the inputs of the transform, and a mirror write that
    survived in another lane's unit (samples 3, 7, 11, ... hold it for a moment) would show there."""
    p = v180_benchmark_params(N, 64, 1)
    assert 0.0 < p.c0 < 1.0
    raw = synthetic_raw(N, 64, 1, seed=41).reshape(-1, N).copy()
    top = 4095
    if bitshift:
        p.bitDepth, p.bitshift = 16, 1
        raw, top = raw16(N, 64, 1, seed=41), 65535
    raw[:, 0], raw[:, 1], raw[:, 2] = 0, top, 0
    raw[:, 3::4] = raw[:, 3::4] // 2  # the words the other lanes' mirror writes pass through differ from sample 1
    run(p, raw, "mirror tap, bitshift %d" % bitshift)


def test_every_bin_in_its_place():
    """white noise: the spectrum of every row differs in every bin, so a bin stored in another bin's place fails the comparison"""
    rng = np.random.default_rng(77)
    p = v180_benchmark_params(N, 64, 1)
    run(p, rng.integers(0, 4096, size=(64, N), dtype=np.uint16), "white-noise rows")


def split(lines):
    """(A-scans per B-scan, B-scans) with the fewest B-scans >= 2 (the flip mirrors even B-scans that have a successor)"""
    for b in range(2, 65):
        if lines % b == 0:
            return lines // b, b
    return lines, 1


@pytest.mark.parametrize("flip", [0, 1])
def test_second_iteration_of_a_wave(flip):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = 8 * cus + 1  # one workgroup of eight waves per CU: exactly one wave runs the loop twice, on a prefetched row
    A, B = split(lines)
    p = v180_benchmark_params(N, A, B)
    p.bscanFlip = flip
    grid = run(p, raw16(N, A, B, seed=17 + flip), "%d lines as %d x %d, flip %d" % (lines, A, B, flip))
    assert grid == cus, "the grid is not one workgroup per CU (%d blocks, %d CUs): the buffer size of this test assumes it" % (grid, cus)


def _lin(p):
    p.signalLogScaling, p.signalGrayscaleMax, p.signalGrayscaleMin = 0, 900.0, 0.0


def _bg(p):
    p.fixedPatternNoiseRemoval, p.postProcessBackgroundRemoval, p.postProcessBackgroundWeight, p.postProcessBackgroundOffset = 0, 1, 0.8, 0.02
    p.signalGrayscaleMax, p.signalGrayscaleMin = 110.0, 20.0
    p.loadPostProcessingBackground(np.linspace(0.0, 0.3, p.samplesPerLine // 2, dtype=np.float32))


def _sinus(p):
    p.sinusoidalScanCorrection = 1


def _roll(p):
    p.bitDepth, p.backgroundRemoval, p.rollingAverageWindowSize = 16, 1, 64


def _real(p):
    p.dispersionCompensation = 0


VARIANTS = {
    # name: (length, settings, path bits the run must show, route flags, clamped image)
    # (the display-fold variants, ROUTE_FUSED_DISPLAY, keep the per-chunk staging and are not among these: csrc/kernels.h)
    "linear_scaling": (1024, _lin, 0, 0, False),
    "background_removal_in_the_store": (1024, _bg, _lib.PATH_FUSED_BG, 0, True),
    "sinusoidal_correction_in_the_store": (1024, _sinus, _lib.PATH_FUSED_SINUS, 0, False),
    "rolling_average_64": (1024, _roll, _lib.PATH_ROLL_IN_KERNEL, 0, False),
    "real_input": (1024, _real, _lib.PATH_REAL_INPUT, 0, False),
    "n256": (256, None, 0, 0, False),
    "n512": (512, None, 0, 0, False),
    "n2048": (2048, None, 0, 0, False),
}


@pytest.mark.parametrize("bitshift", [0, 1])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants_that_share_the_staging(name, bitshift):
    n, settings, path, route, clamped = VARIANTS[name]
    A, B = 32, 2
    p = v180_benchmark_params(n, A, B)
    if n != 1024:
        p.c0, p.c1, p.c2, p.c3 = 0.5, 0.85 * n, -0.17 * n, 0.09 * n  # (the curve tests/test_gpu_parity.py gives the other lengths; it starts below sample 1 too)
    if settings:
        settings(p)
    if bitshift:
        p.bitDepth, p.bitshift = 16, 1
    raw = raw16(n, A, B, seed=500 + n) if p.bitDepth == 16 else synthetic_raw(n, A, B, seed=500 + n).reshape(-1, n)
    run(p, raw, "%s, bitshift %d" % (name, bitshift), path=path, route=route, clamped=clamped)
