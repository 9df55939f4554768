"""Peak analysis on the MI355X against the numpy model on crafted A-scans (tests/peak_cases.py; tests/test_peak_cases.py proves that
each case reaches the branch it declares): every status bit but FIT_STALLED, ties and edges of the argmax, crossings on and next to
the borders of the 64-sample ballot blocks, every group size that takes another path (one pass up to 64, chunk partials with a short
last chunk beyond), windows of 3 .. 65, 1024 / 1025 and 4096 samples, the fit's window and iteration controls; both load forms of
peak_add_rows on the same values; host sources cut into sub-regions and into more than one staging slice.

The averaged A-scans, index, value, position, left, right, fwhm and the status bits of steps 1 to 4 are compared bit for bit, as
include/octpipe.h words it; of the fit, what depends on exact quantities alone (window, FIT_SKIPPED, the number of FIT_* bits, the
flat A-scan that converges at once) is compared exactly, and the parameters after a fixed number of decisive solves within the 1e-7
of tests/test_gpu_peak_analysis.py.

Not covered: the border between two batches of chunk partials (kPartBytes = 64 MiB of float64 partials per batch in
csrc/pipe_peak.hip).  Crossing it takes about 1 GiB of source rows, which is no test of a few seconds."""
import numpy as np
import pytest
import torch

import peak_cases as pc
import peak_model as pm
from octproz_amd import Pipeline, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

EXACT = ("index", "position", "left", "right", "fwhm")
FIT = ("amplitude", "center", "sigma", "offset")
FIT_FLOATS = FIT + ("fitFwhm", "rms")
STAGE_BYTES = 64 << 20  # csrc/pipe_peak.hip: host rows staged per slice

_PIPES = {}
_MODELS = {}
_WORST = {"fit": 0.0, "compared": 0}


def _pipe(shape):
    if shape not in _PIPES:
        _PIPES[shape] = Pipeline(v180_benchmark_params(*shape), device=0)
    return _PIPES[shape]


@pytest.fixture(scope="module", autouse=True)
def _close_pipes():
    yield
    print("crafted peak cases: %d fits compared after a fixed number of solves, worst %.2e of scale" % (_WORST["compared"], _WORST["fit"]))
    for p in _PIPES.values():
        p.close()
    _PIPES.clear()


def _model(case, fit):
    key = (case.name, bool(fit))
    if key not in _MODELS:
        _MODELS[key] = case.model(fit=fit)
    return _MODELS[key]


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _bits(r):
    return [np.ascontiguousarray(getattr(r, f)).view(np.uint8).tobytes() for f in r.FIELDS] + [r.averaged.view(np.uint8).tobytes()]


def _check_group(got, i, j, m, o, what):
    """group (i, j) of a PeakAnalysis with .averaged against the model's averaged A-scan m and its dict o: bit for bit"""
    assert np.array_equal(got.averaged[i, j].view(np.uint32), m.view(np.uint32)), (what, i, j)
    assert (int(got.status[i, j]) & pm.STEP4_BITS) == o["status"] & pm.STEP4_BITS, (what, i, j, got.status[i, j], o["status"])
    assert _same(got.value[i, j], np.float32(o["value"])), (what, i, j, got.value[i, j], o["value"])
    for f in EXACT:
        assert _same(getattr(got, f)[i, j], o[f]), (what, i, j, f, getattr(got, f)[i, j], o[f])


def _check_exact(got, avg, res, what):
    """got: PeakAnalysis with .averaged; avg / res: the model's averaged A-scans and per-group dicts (the check of
    tests/test_gpu_peak_analysis.py)"""
    assert got.averaged.shape == avg.shape, what
    for i, row in enumerate(res):
        for j, o in enumerate(row):
            _check_group(got, i, j, avg[i, j], o, what)


def _check_fit_frame(got, res, fit, what):
    """what of the fit depends on exact quantities alone"""
    for i, row in enumerate(res):
        for j, o in enumerate(row):
            gs = int(got.status[i, j])
            found = not o["status"] & (pm.NO_PEAK | pm.NONFINITE)
            fields = [float(getattr(got, f)[i, j]) for f in FIT_FLOATS]
            if fit and found:
                assert got.fitFirst[i, j] == o["fitFirst"] and got.fitCount[i, j] == o["fitCount"], (what, i, j, got.fitFirst[i, j], got.fitCount[i, j], o)
                assert bin(gs & pm.FIT_BITS).count("1") == 1, (what, i, j, gs)
                assert (gs & pm.FIT_SKIPPED) == (o["status"] & pm.FIT_SKIPPED), (what, i, j, gs, o["status"])
                if gs & pm.FIT_SKIPPED:
                    assert got.iterations[i, j] == 0 and np.all(np.isnan(fields)), (what, i, j)
            else:
                assert not gs & pm.FIT_BITS, (what, i, j, gs)
                assert got.fitFirst[i, j] == 0 and got.fitCount[i, j] == 0 and got.iterations[i, j] == 0, (what, i, j)
                assert np.all(np.isnan(fields)), (what, i, j, fields)


def _check_fit_state(case, got, res, what):
    i, j = case.at
    o = res[i][j]
    if case.fit_exact:
        assert int(got.status[i, j]) == o["status"] and got.iterations[i, j] == o["iterations"], (what, got.status[i, j], o["status"])
        for f in FIT_FLOATS:
            assert _same(getattr(got, f)[i, j], o[f]), (what, f, getattr(got, f)[i, j], o[f])
    it = case.settings["max_iterations"]
    if it:
        assert int(got.status[i, j]) & pm.FIT_BITS == pm.FIT_MAX_ITER and got.iterations[i, j] == it, (what, got.status[i, j], got.iterations[i, j])
    if case.fit_close:
        ref = np.array([o[f] for f in FIT])
        g = np.array([getattr(got, f)[i, j] for f in FIT])
        scale = np.maximum(np.abs(ref), [0.0, ref[2], 0.0, abs(ref[0])])  # (tests/test_gpu_peak_analysis.py::_check_fit)
        dev = float(np.max(np.abs(g - ref) / scale))
        _WORST["fit"], _WORST["compared"] = max(_WORST["fit"], dev), _WORST["compared"] + 1
        print("%s: fit after %d solves, %.2e of scale from the model" % (what, it, dev))
        assert np.all(np.abs(g - ref) <= 1e-7 * scale), (what, g, ref)


def _run_case(pipe, case, data, **over):
    kw = dict(case.settings)
    kw.update(over)
    return pipe.peak_analysis(data=data, averaged=True, **case.region_args(), **kw)


# ------------------------------------------------------------------------------------------------------- a. every case, host and device
@pytest.mark.parametrize("case", pc.cases(), ids=lambda c: c.name)
def test_crafted_case(case):
    pipe = _pipe(case.handle)
    host = case.embed()
    dev = torch.from_numpy(host).cuda()
    fit = case.settings["fit"]
    avg, res = _model(case, fit)
    results = []
    for src, data in (("host", host), ("device", dev)):
        what = (case.name, src)
        got = _run_case(pipe, case, data)
        _check_exact(got, avg, res, what)
        _check_fit_frame(got, res, fit, what)
        _check_fit_state(case, got, res, what)
        results.append(_bits(got))
    assert results[0] == results[1], (case.name, "host and device sources differ")
    assert _bits(_run_case(pipe, case, dev)) == results[1], (case.name, "a repeated call differs")
    if not fit:
        # the instance with the fit runs steps 1 to 4 in its own compiled copy: the same exact results, and a well-formed fit
        avg, res = _model(case, True)
        got = _run_case(pipe, case, dev, fit=True)
        _check_exact(got, avg, res, (case.name, "fit on"))
        _check_fit_frame(got, res, True, (case.name, "fit on"))


# ------------------------------------------------------------------------------------------------------- b. both load forms
def _noisy_peaks(seed, shape, g):
    """rows with a peak whose depth moves from group to group, amplitudes 10**U(0, 4), on noise"""
    rng = np.random.default_rng(seed)
    b, a, s = shape
    z = np.arange(s, dtype=np.float64)
    mu = rng.uniform(0.1 * s, 0.9 * s, size=(b, a // g, 1, 1)).repeat(g, axis=2).reshape(b, a, 1)
    amp = 10 ** rng.uniform(0, 4, size=(b, a, 1))
    return (amp * (np.exp(-0.5 * ((z - mu) / (0.03 * s + 1.0)) ** 2) + 0.05 * rng.random(shape))).astype(np.float32)


@pytest.mark.parametrize("g", [8, 130])
@pytest.mark.parametrize("n", [130, 1024, 2046])
def test_load_forms_give_the_same_bits(n, g):
    """16-byte loads need L % 4 == 0, firstSample % 4 == 0 and an aligned pointer.  L = 512: the aligned tensor takes them, the same
    storage one float further on goes value by value, the staged host copy takes them again.  L = 65 and 1023: rows start at every
    alignment, everything goes value by value.  All equal the model and each other."""
    a, b = 264, 2
    L = n // 2
    pipe = _pipe((n, a, b))
    s0, ns = 4, L - 4 - (L - 4) % 4 - 3  # (the window ends 1 value past a multiple of 4: a 16-byte load reaches 3 values beyond it)
    assert (s0 + ns) % 4 == 1 and s0 + ns < L
    na = 5 * g if g <= 64 else 2 * g
    region = _noisy_peaks(n + g, (2, na, ns), g)
    buf = np.full((b, a, L), np.nan, np.float32)
    buf[:, 3:3 + na, s0:s0 + ns] = region
    need = buf.size
    kw = dict(ascans=(3, na), depth=(s0, ns), ascans_per_group=g, averaged=True)
    aligned = torch.from_numpy(buf).cuda()
    t = torch.full((need + 4,), float("nan"), dtype=torch.float32, device="cuda")
    t[1:1 + need] = aligned.reshape(-1)
    h = np.full(need + 4, np.nan, np.float32)
    h[1:1 + need] = buf.reshape(-1)
    assert aligned.data_ptr() % 16 == 0 and t[1:].data_ptr() % 16 == 4 and h[1:].ctypes.data % 4 == 0
    avg, res = pm.analyse_region(region, g, s0=s0, fit=True)
    got = [pipe.peak_analysis(data=d, **kw) for d in (aligned, t[1:], h[1:])]
    for r, what in zip(got, ("aligned tensor", "tensor one float on", "host array one float on")):
        _check_exact(r, avg, res, (n, g, what))
        _check_fit_frame(r, res, True, (n, g, what))
    assert _bits(got[0]) == _bits(got[1]) == _bits(got[2]), (n, g)


# ------------------------------------------------------------------------------------------------------- c. sub-regions from host memory
@pytest.mark.parametrize("g", [4, 100])
def test_sub_region_from_host_memory(g):
    """every first index non-zero and fewer A-scans than a B-scan has: the staging issues one copy per B-scan"""
    n, a, b = 1024, 208, 3
    pipe = _pipe((n, a, b))
    region = _noisy_peaks(300 + g, (2, 200, 400), g)
    buf = np.full((b, a, n // 2), np.nan, np.float32)
    buf[1:3, 4:204, 5:405] = region
    kw = dict(bscans=(1, 2), ascans=(4, 200), depth=(5, 400), ascans_per_group=g, averaged=True)
    host = pipe.peak_analysis(data=buf, **kw)
    dev = pipe.peak_analysis(data=torch.from_numpy(buf).cuda(), **kw)
    avg, res = pm.analyse_region(region, g, s0=5, fit=True)
    _check_exact(host, avg, res, ("host sub-region", g))
    _check_fit_frame(host, res, True, ("host sub-region", g))
    assert _bits(host) == _bits(dev), g


# ------------------------------------------------------------------------------------------------------- d. beyond one staging slice
def test_host_source_beyond_one_staging_slice():
    """66 MiB of region rows from host memory: G = 64 is staged in slices of whole groups, the border after group 63 inside B-scan 1;
    G = 132 in slices of whole chunks (64, 64, 4 rows), the border inside group 21"""
    n, a, b = 8192, 2120, 2
    depth, fa, na = n // 2, 4, 2112
    rows, row_bytes = b * na, 4 * depth
    assert row_bytes == 16384 and rows * 16384 > STAGE_BYTES
    pipe = _pipe((n, a, b))
    vol = np.random.default_rng(11).standard_normal((b, a, depth), dtype=np.float32)
    vol[:, fa:fa + na] *= (10 ** np.random.default_rng(12).uniform(-2, 3, size=(b, na, 1))).astype(np.float32)
    vol[:, :fa], vol[:, fa + na:] = np.nan, np.nan
    dvol = torch.from_numpy(vol).cuda()
    for g in (64, 132):
        per_bscan, q_all = na // g, b * (na // g)
        if g == 64:
            slice_rows = STAGE_BYTES // row_bytes
            assert slice_rows == 4096 and slice_rows % g == 0 and na < slice_rows < rows  # the border: after group 63, in B-scan 1
            border = [slice_rows // g - 1, slice_rows // g]
        else:
            chunks = -(-g // pm.CHUNK)
            slice_chunks = STAGE_BYTES // (row_bytes * pm.CHUNK)
            assert chunks == 3 and slice_chunks == 64 and 64 % 3 != 0 and slice_chunks < q_all * chunks  # the border: inside group 21
            border = [slice_chunks // chunks - 1, slice_chunks // chunks, slice_chunks // chunks + 1]
        kw = dict(ascans=(fa, na), ascans_per_group=g, fit=False, averaged=True)
        host = pipe.peak_analysis(data=vol, **kw)
        dev = pipe.peak_analysis(data=dvol, **kw)
        assert host.shape == (b, per_bscan)
        assert _bits(host) == _bits(dev), g
        for q in [0] + border + [q_all - 1]:
            i, j = divmod(q, per_bscan)
            m = pm.averaged(vol[i, fa + j * g:fa + (j + 1) * g])
            _check_group(host, i, j, m, pm.analyse(m), ("slices", g, q))


# ------------------------------------------------------------------------------------------------------- e. side conditions
def test_crafted_calls_leave_the_processing_chain_alone():
    """the calls of a. and a host sub-region between two process calls on a live handle: the second image is the one of a handle that
    made no peak calls (the form of tests/test_gpu_peak_analysis.py::test_no_side_effects)"""
    n, a, b = pc.SMALL
    raws = [synthetic_raw(n, a, b, seed=70 + i) for i in range(2)]

    def run(with_peaks):
        pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
        pipe.octCudaPipeline(raws[0])
        pipe.synchronize()
        if with_peaks:
            for case in pc.cases():
                if case.handle != pc.SMALL:
                    continue
                host = case.embed()
                _run_case(pipe, case, host)
                _run_case(pipe, case, torch.from_numpy(host).cuda())
            pipe.peak_analysis(bscans=(1, 2), ascans=(4, 200), depth=(5, 400), ascans_per_group=100)
            pipe.peak_analysis(data=pipe.processed_host(), bscans=(1, 2), ascans=(4, 200), depth=(5, 400), ascans_per_group=4, fit_half_width=7,
                               max_iterations=2, threshold=0.5)
        pipe.octCudaPipeline(raws[1])
        pipe.synchronize()
        out = [pipe.processed_host().copy(), pipe.mean_line().copy()]
        pipe.close()
        return out

    ref, got = run(False), run(True)
    for x, y in zip(ref, got):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
