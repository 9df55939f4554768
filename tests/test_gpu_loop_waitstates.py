"""The kernels whose transform multiplies two complex products per assembly statement (octfft::cmul2 / cmul_const2, fft_pass PAIR in
csrc/kernels.h) against the oracle: the fused kernel and the real-input kernels at N = 256, 1024 and 2048 (N = 512 and the
rolling-average variants of N = 1024 keep the two-statement form and are run along with them).

A paired statement computes the products out of place, two at a time, from the values two registers hold when the statement starts.  What
can go wrong: a pair that takes the wrong partner or the wrong twiddle (one bin group of every A-scan is off), a result register that
overlaps an input (early clobber missing: wrong values in every row), and a packed result consumed before it is written (wrong values in
every row as well).  Every A-scan of every buffer is compared with the frozen policy of tests/common.py, strict (no bin excused), at the
smallest shapes that run each code path twice:

  N x 5 x 2    ten A-scans: fewer than the waves of one workgroup, an odd count per B-scan (the real-input kernels pair rows);
  N x 64 x 3   with ROUTE_TINY_GRID (two workgroups), so that every wave goes round its persistent loop more than once.

Settings: the benchmark's (cubic resampling, dispersion compensation, log scaling), linear resampling, the rolling average of 64 rows
inside the kernel, and dispersion compensation off (the real-input route).  The route each case must take is what csrc/route.h gives
(octpipe_debug_route, tests/test_route.py): path bits 0, 0, ROLL_IN_KERNEL and REAL_INPUT."""
import numpy as np
import pytest

import common
from octproz_amd import Pipeline, _lib, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu


def to_device(raw):
    import torch
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.int16)).to("cuda:0")


def raw16(n, A, B, seed):
    """the benchmark's synthetic fringes moved up to 16 bits with random low bits"""
    rng = np.random.default_rng(seed)
    r = synthetic_raw(n, A, B, seed=seed).astype(np.uint32).reshape(-1, n)
    return (r * 16 + rng.integers(0, 16, size=r.shape, dtype=np.uint32)).astype(np.uint16)


def _bench(p):
    pass


def _linear(p):
    p.resamplingInterpolation = 0


def _roll(p):
    p.bitDepth, p.backgroundRemoval, p.rollingAverageWindowSize = 16, 1, 64


def _real(p):
    p.dispersionCompensation = 0


SETTINGS = {
    # name: (settings, the path bits of the route meant)
    "benchmark": (_bench, 0),
    "linear": (_linear, 0),
    "rolling_average_64": (_roll, _lib.PATH_ROLL_IN_KERNEL),
    "real_input": (_real, _lib.PATH_REAL_INPUT),
}
SHAPES = {"5x2": (5, 2, 0), "64x3_tiny_grid": (64, 3, _lib.ROUTE_TINY_GRID)}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", list(SETTINGS))
@pytest.mark.parametrize("n", [256, 512, 1024, 2048])
def test_paired_multiplies_against_the_oracle(n, name, shape):
    settings, path = SETTINGS[name]
    A, B, route = SHAPES[shape]
    p = v180_benchmark_params(n, A, B)
    if n != 1024:
        p.c0, p.c1, p.c2, p.c3 = 0.5, 0.85 * n, -0.17 * n, 0.09 * n  # (the curve tests/test_gpu_parity.py gives the other lengths)
    settings(p)
    if A * B < 18:
        p.fixedPatternNoiseRemoval = 0  # fewer than 18 lines cannot give a mean line
    p.update_all_curves()
    seed = 900 + n + A
    raw = raw16(n, A, B, seed) if p.bitDepth == 16 else synthetic_raw(n, A, B, seed=seed).reshape(-1, n)
    what = "N = %d, %s, %s" % (n, name, shape)
    o = common.make_oracle(p)
    want = o.process(raw)
    pipe = Pipeline(p, device=0, route=route)
    if p.fixedPatternNoiseRemoval:
        pipe.set_mean_line(o.mean_line(), pin=True)
    d = to_device(raw)
    pipe.process_device(d.data_ptr())
    pipe.synchronize()
    got = pipe.processed_host()
    assert pipe.last_path() == path, "%s: path bits %#x, meant %#x" % (what, pipe.last_path(), path)
    if route and not path & _lib.PATH_REAL_INPUT:  # (the launchers of the real-input kernels do not report their grid)
        assert pipe.last_grid() == 2, "%s: %d workgroups" % (what, pipe.last_grid())
    rel, db = common.compare_images(got, want, p, what, strict=True, mean_line=o.mean_line())
    print("%s: max linear-power error %.2e, max normalised-dB error %.2e" % (what, rel, db))
    pipe.close(); o.close()
