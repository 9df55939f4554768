"""Phase extraction on the MI355X on the crafted inputs of tests/phase_cases.py (tests/test_phase_cases.py proves on the model that
each case reaches what it declares).

1. accumulate: every instance of oct_phase_accumulate_kernel<F, VEC> (8 formats x vector / scalar) and every launch shape of
   launchAccumulate -- column blocks, rows side by side with and without idle threads, row groups, every tail behind the unrolled
   loop, a row count below rowsPerPass, a misaligned device base -- on random samples, on the formats' extremes and on rows of a
   constant.  The mean is bit-equal to float32((int64 sum / count) * scale) of the decoded integers, the source is left untouched
   (the marker bytes around a sliced source included), a second handle fed the same rows in fewer calls from the other memory gives
   the same bits.
2. packed 12 bit on rows of odd length (every odd row starts inside a byte triple; csrc/phase_stage.h), host against device.
3. extract: means whose phase is not monotone, so that the prefix-max / suffix-min scans across lanes and both clamps of the inversion
   work.  The curve is judged by its forward residual |psi_mono(curve[j]) - j| against the float64 model's psi_mono: on a flat
   stretch of psi_mono the curve itself jumps by the stretch's length for an infinitesimal change of level, the residual does not.

Not covered: the int32 partial flush every PHASE_TILE = 16384 rows of a lane (with up to 8 row groups per CU that takes about 10^7
A-scans in one call); the border between two 64 MiB staging slices of the host path (its arithmetic is checked on the host by
tests/native/phase_stage_check.cpp with small budgets); kMaxAscans."""
import numpy as np
import pytest
import torch

import phase_cases as pc
import phase_model as pm
from octproz_amd import OctAlgorithmParameters, OctPipeError, Pipeline
from test_gpu_phase_extraction import CURVE_ATOL, SPECTRUM_RTOL

pytestmark = pytest.mark.gpu

MARKER = 0xA5


def _pipe(n, a, b, fmt=0, bit_depth=12, bitshift=0):
    p = OctAlgorithmParameters()
    p.samplesPerLine, p.ascansPerBscan, p.bscansPerBuffer, p.bitDepth = n, a, b, bit_depth
    p.bitshift = bitshift
    p.update_all_curves()
    return Pipeline(p, device=0, sample_format=fmt)


class _Sources:
    """the three memories of one raw buffer: the host array, an aligned device tensor, a device tensor `offset` bytes into an aligned
    allocation with marker bytes around the data"""

    def __init__(self, raw, offset):
        self.host = np.ascontiguousarray(raw)
        self.bytes = self.host.reshape(-1).view(np.uint8)
        self.offset = offset
        self._dev = self._alloc = None

    def get(self, source):
        if source == "host":
            return self.host
        if source == "device":
            if self._dev is None:
                self._dev = torch.from_numpy(self.bytes.copy()).cuda()
                assert self._dev.data_ptr() % 16 == 0
            return self._dev
        if self._alloc is None:
            t = torch.full((self.bytes.size + 64,), MARKER, dtype=torch.uint8, device="cuda")
            t[self.offset:self.offset + self.bytes.size] = torch.from_numpy(self.bytes.copy()).cuda()
            assert t.data_ptr() % 16 == 0
            self._alloc = t
        cut = self._alloc[self.offset:]
        assert cut.data_ptr() == self._alloc.data_ptr() + self.offset and cut.is_contiguous()
        return cut

    def assert_untouched(self, name):
        if self._dev is not None:
            assert np.array_equal(self._dev.cpu().numpy(), self.bytes), name
        if self._alloc is not None:
            got = self._alloc.cpu().numpy()
            o, k = self.offset, self.bytes.size
            assert np.array_equal(got[o:o + k], self.bytes), name
            assert np.all(got[:o] == MARKER) and np.all(got[o + k:] == MARKER), name


def _feed(pipe, src, calls, timed=False):
    pipe.phase_reset()
    ms = []
    for first, count, source in calls:
        if timed:
            ms.append(pipe.phase_accumulate_timed(src.get(source), first, count))
        else:
            pipe.phase_accumulate(src.get(source), first, count)
    return pipe.phase_mean(), ms


def _run_accumulate(case, timed=False):
    raw, dec = case.data()
    src = _Sources(raw, pc.misaligned_offset(case.fmt, case.bit_depth))
    want, count = case.expected(dec)
    pipes = [_pipe(case.n, case.a, case.b, case.fmt, case.bit_depth, case.bitshift) for _ in range(2)]
    try:
        for source in {s for _, _, s in case.calls + case.twin_calls()} - {"host"}:  # the launch forms the table was proved for
            base = src.get(source).data_ptr()
            assert base % 16 == (src.offset if source == "sliced" else 0)
        (m, c), _ = _feed(pipes[0], src, case.calls)
        assert c == count
        assert np.array_equal(m.view(np.uint32), want.view(np.uint32)), (case.name, int(np.count_nonzero(m != want)))
        (m2, c2), _ = _feed(pipes[1], src, case.twin_calls())
        assert c2 == count and np.array_equal(m2.view(np.uint32), m.view(np.uint32)), case.name
        if timed:
            (m3, c3), ms = _feed(pipes[1], src, case.calls, timed=True)
            assert all(t > 0.0 for t in ms) and len(ms) == len(case.calls), ms
            assert c3 == count and np.array_equal(m3.view(np.uint32), m.view(np.uint32)), case.name
        src.assert_untouched(case.name)
    finally:
        for p in pipes:
            p.close()


TIMED = {"vector-u16-1024", "scalar-p12s-1024"}
assert TIMED <= {c.name for c in pc.ACCUMULATE_CASES}


# ---------------------------------------------------------------------------------------------------------------------- 1. accumulate
@pytest.mark.parametrize("case", pc.ACCUMULATE_CASES, ids=repr)
def test_accumulate_case(case):
    _run_accumulate(case, timed=case.name in TIMED)


# ---------------------------------------------------------------------------------------------------------------------- 2. packed, odd N
def _odd_handle(fmt, n, a, b):
    """a handle of the odd length n or, should this machine have no route for it, of the nearest odd length that has one"""
    last = None
    for m in (n, n + 2, n - 2, n + 4, n - 4):
        try:
            return m, _pipe(m, a, b, fmt, 12)
        except OctPipeError as e:
            last = e
    raise last


def test_packed_rows_of_odd_length():
    """Formats 1 and 2 at N = 129 (4 x 2 A-scans) and N = 255 (2 x 3): calls that start at A-scans 0, 1, 2 and 3 and the whole
    buffer.  On a host buffer every odd row starts inside a byte triple, which the host path's staging has to follow: host against
    the model, device against the model, and one host call against several."""
    for fmt, n, a, b in pc.PACKED_ODD:
        n, pipe = _odd_handle(fmt, n, a, b)
        try:
            host, dev = pc.packed_odd_case(fmt, n, a, b, "host"), pc.packed_odd_case(fmt, n, a, b, "device")
            raw, dec = host.data()
            src = _Sources(raw, 3)
            for case in (host, dev):
                assert not case.form()[0]
                want, count = case.expected(dec)
                (m, c), _ = _feed(pipe, src, case.calls)
                assert c == count and np.array_equal(m.view(np.uint32), want.view(np.uint32)), (case.name, int(np.count_nonzero(m != want)))
                # every call on its own
                for call in case.calls:
                    want1, count1 = case.expected(dec, [call])
                    (m1, c1), _ = _feed(pipe, src, [call])
                    assert c1 == count1 and np.array_equal(m1.view(np.uint32), want1.view(np.uint32)), (case.name, call)
            lines = a * b
            (whole, _), _ = _feed(pipe, src, [(0, lines, "host")])
            (parts, _), _ = _feed(pipe, src, [(0, 1, "host"), (1, 1, "host"), (2, lines - 3, "host"), (lines - 1, 1, "host")])
            (sliced, _), _ = _feed(pipe, src, [(0, 3, "sliced"), (3, lines - 3, "sliced")])
            assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32)) and np.array_equal(whole.view(np.uint32), sliced.view(np.uint32))
            src.assert_untouched((fmt, n))
        finally:
            pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 3. extract
_EXTRACT_PIPES = {}


@pytest.fixture(scope="module")
def extract_pipe():
    def get(n):
        if n not in _EXTRACT_PIPES:
            _EXTRACT_PIPES[n] = _pipe(n, 32, 2)
        return _EXTRACT_PIPES[n]
    yield get
    for p in _EXTRACT_PIPES.values():
        p.close()
    _EXTRACT_PIPES.clear()


DEVICE_RESIDUALS = {}


@pytest.mark.parametrize("case", pc.EXTRACT_CASES, ids=repr)
def test_extract_case(case, extract_pipe):
    n, a, b = case.n, case.a, case.b
    pipe = extract_pipe(n)
    mean = case.mean()
    res = pipe.extract_resample_curve(mean=mean, **case.kwargs())
    want = case.model()
    mono = want["psi_mono"]
    j = np.arange(n, dtype=np.float64)
    es = np.abs(res.spectrum - want["spectrum"]).max() / want["spectrum"].max()
    ee = np.abs(res.envelope - want["envelope"]).max() / want["envelope"].max()
    curve = res.curve.astype(np.float64)
    inside = pc.domain(mono, n)
    near = pc.near_clamp(mono, n, CURVE_ATOL)
    residual = np.abs(pm.forward(mono, curve) - j)
    clamped = np.where(j < mono[0], curve == 0.0, curve == float(n - 1))
    worst = residual[inside & ~near].max()
    DEVICE_RESIDUALS[case.name] = worst
    print("%s: spectrum %.2e, envelope %.2e, forward residual %.2e sample over %d entries, %d below / %d above the levels, %d near a border"
          % (case.name, es, ee, worst, int((inside & ~near).sum()), int((j < mono[0]).sum()), int((j >= mono[-1]).sum()), int(near.sum())))
    assert es <= SPECTRUM_RTOL and ee <= SPECTRUM_RTOL * 10, (case.name, es, ee)
    assert worst <= CURVE_ATOL, (case.name, worst)
    assert np.all(clamped[~inside & ~near]), (case.name, np.nonzero(~clamped & ~inside & ~near)[0][:8])
    assert np.all(clamped[near] | (residual[near] <= CURVE_ATOL)) and int(near.sum()) <= 4, case.name
    assert np.all(np.diff(res.curve) >= 0), case.name
    np.testing.assert_allclose(res.coeffs, pm.fit_cubic(res.curve, a, b), rtol=1e-5, atol=1e-3)
    again = pipe.extract_resample_curve(mean=mean, **case.kwargs())
    for f in ("spectrum", "envelope", "phase", "curve", "coeffs"):
        assert np.array_equal(getattr(res, f).view(np.uint32), getattr(again, f).view(np.uint32)), (case.name, f)


@pytest.mark.parametrize("n", pc.LENGTHS)
def test_no_calibration_signal_in_a_band_without_a_tone(n, extract_pipe):
    case = pc.silent_band_case(n)
    with pytest.raises(OctPipeError) as e:
        extract_pipe(n).extract_resample_curve(mean=case.mean(), **case.kwargs())
    assert e.value.code == 1 and "no calibration signal" in str(e.value)
    # the same mean with the band on the lower tone is a signal
    res = extract_pipe(n).extract_resample_curve(mean=case.mean(), peak=(n // 4 - 10, n // 4 + 10), ignore_first=case.a, ignore_last=n - 1 - case.b)
    assert np.all(np.isfinite(res.curve))
