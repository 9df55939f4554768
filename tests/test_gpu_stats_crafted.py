"""Image statistics on the MI355X against the numpy model on crafted regions (tests/stats_cases.py; tests/test_stats_cases.py proves that
each case reaches the path it declares): 1. the vector loads with a masked tail and the scalar form behind a misaligned device base, in
every container; 2. more segments than workgroups, under both caps; 3. host sources staged in two slices whose border lies inside a
B-scan, float32 and packed 12 bit on odd rows; 4. the wave-uniform histogram add with inactive lanes, lane 0 among them, and waves split
by one lane; 5. the correction of the raw bin quotient and the float32 binning at the ends of its range; 6. moments of data with a large
mean and a small spread.

Histogram and counts bit-exact against tests/stats_model.py, min / max equal, mean and stddev within the 1e-9 of
tests/test_gpu_image_statistics.py (its _check, imported), host and device sources, repeats and both handle sizes bit-equal (its _same_bits).

Not covered: the `values >> 31` term of groupCap (csrc/pipe_stats.hip), which takes more than 2**31 values; the q-- of stats_bin_raw
(csrc/image_stats.h): with d < 2**44 and q * width <= d the float64 product d * (1 / width) is within q * 2**-51 < 1 / width of the true
quotient, so it never reaches the next integer from below it and the truncation is never too large."""
import numpy as np
import pytest
import torch

import stats_cases as sc
from octproz_amd import Pipeline, v180_benchmark_params
from test_gpu_image_statistics import MOMENT_RTOL, _check, _same_bits

pytestmark = pytest.mark.gpu

assert MOMENT_RTOL == 1e-9

_PIPES = {}
_SHARED = {}


def _pipe(handle, fmt, bitshift=0):
    key = (handle, fmt, bitshift)
    if key not in _PIPES:
        p = v180_benchmark_params(*handle)
        if fmt == sc.F32:
            _PIPES[key] = Pipeline(p, device=0)
        else:
            p.bitDepth, p.bitshift = fmt[1], bitshift
            p.update_all_curves()
            _PIPES[key] = Pipeline(p, device=0, sample_format=fmt[0])
    return _PIPES[key]


def _close(handle):
    for key in [k for k in _PIPES if k[0] == handle]:
        _PIPES.pop(key).close()


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for p in _PIPES.values():
        p.close()
    _PIPES.clear()
    _SHARED.clear()


def _shared(key, make):
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def _call(case, data, bins, rng):
    pipe = _pipe(case.handle, case.fmt, case.bitshift)
    kw = case.call_args(bins, rng)
    return pipe.processed_statistics(data=data, **kw) if case.fmt == sc.F32 else pipe.raw_statistics(data, **kw)


def _aligned(source):
    t = torch.from_numpy(source).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _shifted(source, off):
    """the same bytes in device memory `off` bytes past a 16-byte border, poison bytes around them"""
    raw = torch.from_numpy(source.reshape(-1).view(np.uint8))
    t = torch.full((raw.numel() + 64,), 0xFF, dtype=torch.uint8, device="cuda")  # (0xFFFFFFFF is a NaN)
    t[off:off + raw.numel()] = raw.cuda()
    assert t.data_ptr() % 16 == 0
    cut = t[off:]
    if source.dtype == np.float32:
        assert off % 4 == 0
        cut = cut[:(cut.numel() // 4) * 4].view(torch.float32)
    assert cut.data_ptr() == t.data_ptr() + off and cut.is_contiguous()
    return cut


def _run(case, whole=None, host=None, dev=None):
    """every (bins, range) of a case from a host and a device source: the model's bits, and the same bits from both"""
    whole = case.whole() if whole is None else whole
    host = case.source(whole) if host is None else host
    dev = _aligned(host) if dev is None else dev
    values = case.values(whole)
    out = []
    for bins, rng in case.runs:
        want = case.model(values, bins, rng)
        got = _call(case, dev, bins, rng)
        _check(got, want, (case.name, bins, rng, "device"))
        _same_bits(got, _call(case, host, bins, rng), (case.name, bins, rng, "host against device"))
        out.append((got, want))
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. load forms
@pytest.mark.parametrize("fmt,bitshift", [(f, s) for f in sc.LOAD_FORMATS for s in ((0, 1) if sc.has_bitshift(f) else (0,))],
                         ids=lambda x: "shift%d" % x if isinstance(x, int) else sc.FORMAT_ID[x])
def test_load_forms_and_misaligned_bases(fmt, bitshift):
    """windows on multiples of V with 1, V - 1, V, V + 1, 2V + 3 values and to the row's end take the vector form from the aligned
    tensor and the staged host copy and the scalar form from every misaligned base; their twins one sample on take the scalar form"""
    for case in sc.load_form_cases(fmt, bitshift):
        whole = case.whole()
        host = case.source(whole)
        values = case.values(whole)
        aligned = _aligned(host)
        assert case.plan.vector_form(aligned.data_ptr()) == case.expect["vector"]
        moved = []
        for off in sc.load_offsets(fmt):
            t = _shifted(host, off)
            assert not case.plan.vector_form(t.data_ptr())
            moved.append(t)
        for bins, rng in case.runs:
            want = case.model(values, bins, rng)
            got = _call(case, aligned, bins, rng)
            _check(got, want, (case.name, bins, rng))
            _same_bits(got, _call(case, host, bins, rng), (case.name, bins, rng, "host"))
            for off, t in zip(sc.load_offsets(fmt), moved):
                _same_bits(got, _call(case, t, bins, rng), (case.name, bins, rng, "base + %d bytes" % off))


# ---------------------------------------------------------------------------------------------------------------- 2. segment grid
@pytest.mark.parametrize("case", sc.grid_cases(), ids=repr)
def test_more_segments_than_workgroups(case):
    p, e = case.plan, case.expect
    bins = case.runs[0][0]
    assert (p.G, p.seg_rows, p.segments, p.groups(bins)) == (e["G"], e["seg_rows"], e["segments"], e["groups"])
    assert (p.segments > p.group_cap(bins)) == (bins != 512)
    whole = _shared(("grid", case.fmt), case.whole)
    host = _shared(("grid host", case.fmt), lambda: case.source(whole))
    dev = _shared(("grid device", case.fmt), lambda: _aligned(host))
    for got, want in _run(case, whole, host, dev):
        # every segment's values are counted once: a workgroup that skipped its second segment would lose counts
        total = int(got.histogram.sum()) + got.underflow + got.overflow
        assert total == got.count == p.rows * case.window[1] - got.nonFinite


# ---------------------------------------------------------------------------------------------------------------- 3. staging slices
def test_float_host_source_in_two_slices():
    case = sc.slice_cases()[0]
    p = case.plan
    assert case.fmt == sc.F32 and p.slice_borders() == [4080] and 4080 % case.ascans[1] != 0 and p.vector_form(staged=True)
    try:
        _run(case)
    finally:
        _close(case.handle)


@pytest.mark.parametrize("fmt", [(1, 12), (2, 12)], ids=["p12u", "p12s"])
def test_packed_host_source_in_two_slices(fmt):
    """73 MiB of random packed bytes on rows of 1001 samples: every B-scan run is staged on its own sample parity, the second slice
    begins 448 rows into B-scan 86 (with 500 of the 512 A-scans: 480 rows into B-scan 88)"""
    cases = [c for c in sc.slice_cases() if c.fmt == fmt]
    assert len(cases) == 2
    host = _shared("packed bytes", cases[0].whole)
    dev = _shared("packed device", lambda: _aligned(host))
    try:
        for case in cases:
            p = case.plan
            assert p.parity() and p.seg_rows == 32 and p.slice_segments() == 1390 and p.slice_borders() == [44480]
            assert 44480 % case.ascans[1] == case.expect["border_in_bscan"]
            _run(case, host, host, dev)
    finally:
        _close(cases[0].handle)


# ---------------------------------------------------------------------------------------------------------------- 4. wave-uniform add
@pytest.mark.parametrize("case", sc.wave_cases(), ids=repr)
def test_wave_uniform_add(case):
    assert case.plan.vector_form(0) and case.window[1] % case.plan.V != 0
    _run(case)


# ---------------------------------------------------------------------------------------------------------------- 5. binning edges
@pytest.mark.parametrize("case", sc.raw_edge_cases(), ids=repr)
def test_raw_bin_edges(case):
    _run(case)


@pytest.mark.parametrize("case", sc.processed_edge_cases(), ids=repr)
def test_processed_bin_edges(case):
    _run(case)


# ---------------------------------------------------------------------------------------------------------------- 6. moments
@pytest.mark.parametrize("kind", [k for k, _ in sc.MOMENT_KINDS])
def test_moments_of_a_large_mean_and_a_small_spread(kind):
    whole32, sub32, sub48 = [c for c in sc.moment_cases() if c.expect["kind"] == kind]
    got = {}
    for case in (whole32, sub32, sub48):
        whole = case.whole()
        host = case.source(whole)
        dev = _aligned(host)
        (first, want), = _run(case, whole, host, dev)
        bins, rng = case.runs[0]
        _same_bits(first, _call(case, dev, bins, rng), (case.name, "repeat"))
        print("%s: mean %.17g (numpy %.17g), stddev %.17g (numpy %.17g)" % (case.name, first.mean, want["mean"], first.stddev, want["stddev"]))
        got[case.name] = first
    _same_bits(got[sub32.name], got[sub48.name], (kind, "the same region in handles of 32 and 48 A-scans"))
