"""Repeat registration on the MI355X (include/octpipe.h "repeat registration", csrc/repeat_register.h, csrc/pipe_angio.hip).

Every result is compared bit for bit against the numpy model of tests/register_model.py (integers as they are, floats as uint32, costs as
uint64): there is no tolerance and nothing is excused.  The shapes are those of tests/test_gpu_angiogram.py (ascanCount 1, 67, 130 and the
handle with an odd depth), every one with at least two positions; a handle with a depth of 4096 carries maxShift = 64 and the search
kernel's largest LDS allocation.

The volumes are shifted copies of one long random profile per A-scan plus independent noise, so the true shifts (0, +8 and -8 among
them) are known, and continuous random data leaves no accidental tie between two lags; the tie rule has a crafted volume of its own.
The model's registered volume is worked out once per (volume, region, M, method, shifts) without the mask and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import angio_model as am
import register_model as rm
from octproz_amd import OctPipeError, Pipeline, _lib, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

METHODS = ((0, "variance"), (1, "decorrelation"), (2, "difference"))
MARK = -77.0
RVOL = 8  # the largest true shift of the test volumes


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    g, w = np.ascontiguousarray(got).view(view), np.ascontiguousarray(want).view(view)
    if not np.array_equal(g, w):
        i = np.argwhere(g != w)
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %s (%#x), want %s (%#x)" % (
            what, len(i), g.size, tuple(i[0]), got[tuple(i[0])], g[tuple(i[0])], want[tuple(i[0])], w[tuple(i[0])]))


def _dev(raw):
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.int16)).to("cuda:0")


def _guarded(shape, dtype=torch.float32):
    """(pad, view): a device result inside a marked buffer with 8 guard elements on either side, the fill finished before the handle's stream
    writes there"""
    count = int(np.prod(shape))
    pad = torch.full((count + 16,), MARK, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return pad, pad[8:8 + count].view(shape)


def _guards_intact(pad, what):
    host = pad.cpu().numpy()
    assert np.all(host[:8] == MARK) and np.all(host[-8:] == MARK), ("written outside the result", what)


def _host(pipe, tensor):
    pipe.synchronize()
    return tensor.cpu().numpy()


def _moving_volume(b, a, depth, M, seed):
    """(volume float32 [b][a][depth], true shifts [b // M][M]): repeat m of position p shows bin s of the A-scan's long profile at bin
    s + delta[p][m], plus noise of 3 % of its spread; repeat 1 of the first three positions moves by +8 / -8 / 0.  One NaN in the first
    A-scan and one inf in the last make their groups non-finite."""
    rng = np.random.default_rng(seed)
    P = b // M
    delta = rng.integers(-RVOL, RVOL + 1, (P, M))
    delta[:, 0] = 0
    for p, d in zip(range(P), (RVOL, -RVOL, 0)):
        delta[p, 1] = d
    vol = np.zeros((b, a, depth), np.float32)
    for p in range(P):
        base = rng.standard_normal((a, depth + 2 * RVOL)).astype(np.float32)
        for m in range(M):
            d = int(delta[p, m])
            vol[p * M + m] = base[:, RVOL - d:RVOL - d + depth] + (0.03 * rng.standard_normal((a, depth))).astype(np.float32)
    vol[min(3, P - 1) * M + 1, 0, 2] = np.nan      # repeat 1 of position 3 (or the last), first A-scan, outside every inner window here
    vol[(P - 1) * M, a - 1, depth // 2] = np.inf   # repeat 0 of the last position, last A-scan
    return vol, delta


def _kw(region):
    b0, bn, a0, an, s0, sn = region
    return dict(bscans=(b0, bn), ascans=(a0, an), depth=(s0, sn))


def _odd_depth_handle(a, b):
    for n in [250] + list(range(6, 250, 4)):
        try:
            return Pipeline(v180_benchmark_params(n, a, b), device=0), n
        except OctPipeError:
            continue
    raise AssertionError("no samplesPerLine with an odd N / 2 is accepted")


# (N, A, B, M of the volume's true shifts): the (M, (firstBscan, bscanCount)) combinations, every one with at least two positions, and the
# (firstAscan, ascanCount, G) combinations: G = 1, a divisor below 64, the whole range; 67, 65 and 130 cross the chunk of 64 A-scans, 4 and 8
# lie on either side of the group size from which the search runs four waves per group
SHAPES = [
    (256, 1, 16, 2, ((2, (0, 16)), (3, (0, 6)), (8, (0, 16)), (2, (4, 8))), ((0, 1, 1),)),
    (256, 67, 6, 3, ((3, (0, 6)), (2, (0, 6)), (2, (2, 4))), ((0, 67, 1), (0, 67, 67), (2, 64, 32), (1, 66, 33), (3, 64, 64))),
    (256, 130, 4, 2, ((2, (0, 4)),), ((0, 130, 1), (0, 130, 26), (0, 130, 65), (0, 130, 130), (1, 128, 128))),
    ("odd", 9, 15, 3, ((3, (0, 15)), (5, (0, 15)), (3, (6, 9))), ((0, 9, 1), (0, 9, 3), (0, 9, 9), (1, 8, 2), (1, 8, 4), (1, 8, 8))),
]


class Small:
    def __init__(self, pipe, vol, delta, vm, combos, groups):
        self.pipe, self.vol, self.delta, self.vm, self.combos, self.groups = pipe, vol, delta, vm, combos, groups
        self.dvol = torch.from_numpy(vol).cuda()
        self._ref = {}

    def registered(self, region, M, method, shifts, G):
        """the model's registered (contrast, mean, covered) of a region without the mask, fill = MARK: computed once, never changed"""
        key = (region, M, method, shifts.tobytes(), G)
        if key not in self._ref:
            out, mean = rm.angiogram_registered(self.vol, region, M, method, shifts, G, MARK)
            b0, bn, a0, an, s0, sn = region
            cov = np.zeros(out.shape, bool)
            for p in range(out.shape[0]):
                for a in range(an):
                    lo, hi = rm.covered(shifts.reshape(out.shape[0], M, -1)[p, :, a // G], s0, sn)
                    if lo <= hi:
                        cov[p, a, lo - s0:hi - s0 + 1] = True
            for x in (out, mean, cov):
                x.setflags(write=False)
            self._ref[key] = (out, mean, cov)
        return self._ref[key]

    def expected(self, region, M, method, shifts, G, fill, threshold=None, masked=0.0):
        out, mean, cov = self.registered(region, M, method, shifts, G)
        res = out.copy()
        if threshold is not None:
            res[cov] = am.apply_mask(out, mean, threshold, masked)[cov]
        res.view(np.uint32)[~cov] = np.float32(fill).view(np.uint32)
        mu = mean.copy()
        mu.view(np.uint32)[~cov] = np.float32(fill).view(np.uint32)
        return res, mu


@pytest.fixture(scope="module", params=SHAPES, ids=["1x16", "67x6", "130x4", "odd-depth"])
def small(request):
    n, a, b, vm, combos, groups = request.param
    if n == "odd":
        pipe, n = _odd_depth_handle(a, b)
        assert (n // 2) % 2 == 1
    else:
        pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    vol, delta = _moving_volume(b, a, n // 2, vm, seed=a * 5 + b)
    yield Small(pipe, vol, delta, vm, combos, groups)
    pipe.close()


def _windows(depth, R):
    """(firstSample, sampleCount): K = 1, K below 64, K = 64 and K = 64 k + 3 where the depth allows, odd and even starts, the whole depth"""
    w = [(1, 2 * R + 1), (3, 2 * R + 20), (0, depth), (depth - (2 * R + 5), 2 * R + 5)]
    for K in (64, 67):
        if K + 2 * R <= depth - 1:
            w.append((1, K + 2 * R))
    return w


def _crafted_shifts(rng, P, M, Qp, sn):
    """any values: lags around zero, a non-zero entry for m = 0, one group whose repeats leave nothing covered, one beyond the window"""
    s = rng.integers(-5, 6, (P, M, Qp)).astype(np.int32)
    s[:, 0] = 0
    s[0, 0, 0] = 3
    if Qp > 1:
        s[P - 1, :, Qp - 1] = 2  # every repeat alike: Wc only moves
    if P > 1:
        s[1, 1, 0], s[1, 0, 0] = sn, 0  # nothing covered
    if Qp > 2:
        s[0, M - 1, 1] = -2 ** 31
        s[0, 0, 2] = 2 ** 31 - 1
    return s


# ---------------------------------------------------------------------------------------------------------------------- 1. the estimate
def test_the_true_shifts_are_recovered(small):
    """the test volumes are meaningful: with one group per B-scan and R = 8 the model finds the shifts the volume was built with (B-scans with
    a non-finite value apart: the first and the last A-scan hold them and are left out where there are others), and so does the device"""
    b, a, depth = small.vol.shape
    M = small.vm
    a0, an = (1, a - 2) if a >= 3 else (0, a)
    region = (0, b, a0, an, 0, depth)
    want, _, _ = rm.repeat_shifts(small.vol, region, M, an, RVOL)
    finite = np.isfinite(small.vol[:, a0:a0 + an]).all(axis=(1, 2)).reshape(b // M, M)
    ok = finite & finite[:, :1]
    assert {RVOL, -RVOL} <= set(small.delta[ok].tolist())
    assert np.array_equal(want[:, :, 0][ok], small.delta[ok]) and not want[:, :, 0][~ok].any()
    _same(small.pipe.register_repeats(M, max_shift=RVOL, data=small.dvol, **_kw(region)), want, "true shifts")


def test_estimate_small_shapes(small):
    pipe, vol, dvol = small.pipe, small.vol, small.dvol
    b, a, depth = vol.shape
    k = 0
    seen = set()
    for M, (b0, bn) in small.combos:
        for a0, an, G in small.groups:
            for R in (1, 8):
                for s0, sn in _windows(depth, R):
                    k += 1
                    region = (b0, bn, a0, an, s0, sn)
                    want, want_costs, _ = rm.repeat_shifts(vol, region, M, G, R)
                    what = (region, M, G, R)
                    mode = k % 4
                    seen.add((mode, G > 64, sn - 2 * R in (1, 64, 67)))
                    kw = dict(ascans_per_group=G, max_shift=R, **_kw(region))
                    if mode == 0:    # device source, host result, with costs
                        got, costs = pipe.register_repeats(M, costs=True, data=dvol, **kw)
                    elif mode == 1:  # host source (staged), host result, with costs
                        got, costs = pipe.register_repeats(M, costs=True, data=vol, **kw)
                    elif mode == 2:  # device source, device results between guards
                        spad, sout = _guarded(want.shape, torch.int32)
                        cpad, cout = _guarded(want_costs.shape, torch.float64)
                        res = pipe.register_repeats(M, costs=cout, data=dvol, out=sout, **kw)
                        assert res[0] is sout and res[1] is cout
                        got, costs = _host(pipe, sout), cout.cpu().numpy()
                        _guards_intact(spad, what)
                        _guards_intact(cpad, what)
                    else:            # host source, device shifts, no costs
                        spad, sout = _guarded(want.shape, torch.int32)
                        assert pipe.register_repeats(M, data=vol, out=sout, **kw) is sout
                        got, costs = _host(pipe, sout), None
                        _guards_intact(spad, what)
                    _same(got, want, ("shifts", mode) + what)
                    if costs is not None:
                        _same(costs, want_costs, ("costs", mode) + what)
    assert {m for m, _, _ in seen} == {0, 1, 2, 3}
    _same(_host(pipe, dvol), vol, "the source volume")


def test_the_profiles_are_the_peak_analysis_averaged_ascans(small):
    pipe, vol, dvol = small.pipe, small.vol, small.dvol
    b, a, depth = vol.shape
    M, (b0, bn) = small.combos[0]
    for a0, an, G in small.groups:
        region = (b0, bn, a0, an, 1, depth - 3)
        _, _, prof = rm.repeat_shifts(vol, region, M, G, 1)
        avg = pipe.peak_analysis(data=dvol, ascans_per_group=G, fit=False, averaged=True, **_kw(region)).averaged
        _same(np.asarray(avg).reshape(prof.shape), prof, ("profiles", region, G))


def test_tie_rule_and_non_finite_values_on_the_device():
    n, a, b, R = 256, 2, 4, 4
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    depth, c = n // 2, 40
    vol = np.zeros((b, a, depth), np.float32)
    vol[0, :, c] = 1.0
    vol[1, :, c - 2] = vol[1, :, c + 2] = 1.0   # position 0: C(-2) = C(+2) = 1, the other lags 3
    vol[2:] = 2.5                               # position 1: constant profiles, every lag 0
    vol[3, 1, 5] = -np.inf
    for G in (1, 2):
        region = (0, b, 0, a, 3, 90)
        want, want_costs, _ = rm.repeat_shifts(vol, region, 2, G, R)
        assert np.all(want[0, 1] == -2) and np.all(want_costs[0, 0, :, R - 2] == 1.0) and np.all(want_costs[0, 0, :, R] == 3.0)
        assert not want[1].any() and np.all(want_costs[1, 0, -1].view(np.uint64) == rm.CANONICAL_NAN64)
        for data in (vol, torch.from_numpy(vol).cuda()):
            got, costs = pipe.register_repeats(2, G, R, costs=True, data=data, **_kw(region))
            _same(got, want, ("tie", G))
            _same(costs, want_costs, ("tie costs", G))
    pipe.close()


def test_max_shift_64_and_the_deepest_window():
    """depth 4096, M = 8: the search kernel's largest LDS allocation (128 KiB of profiles and the costs of 903 pairs, beyond the 64 KiB a
    kernel gets without asking), R = 64 with K = 1 and K = 3968"""
    n, a, b, M = 8192, 3, 16, 8
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    vol, _ = _moving_volume(b, a, n // 2, M, seed=9)
    dvol = torch.from_numpy(vol).cuda()
    for region, G, R in (((0, b, 0, a, 0, 4096), 1, 64), ((0, b, 0, a, 0, 4096), 3, 64), ((8, 8, 0, a, 7, 129), 3, 64), ((0, b, 1, 2, 100, 1500), 1, 33)):
        want, want_costs, _ = rm.repeat_shifts(vol, region, M, G, R)
        spad, sout = _guarded(want.shape, torch.int32)
        cpad, cout = _guarded(want_costs.shape, torch.float64)
        pipe.register_repeats(M, G, R, costs=cout, data=dvol, out=sout, **_kw(region))
        _same(_host(pipe, sout), want, ("shifts", region, G, R))
        _same(cout.cpu().numpy(), want_costs, ("costs", region, G, R))
        _guards_intact(spad, region)
        _guards_intact(cpad, region)
    got = pipe.register_repeats(M, 3, 64, data=vol)
    _same(got, rm.repeat_shifts(vol, (0, b, 0, a, 0, 4096), M, 3, 64)[0], "host source")
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 2. the registered volume
def _registered_cases(small):
    """(region, M, G, estimated shifts, crafted shifts) of the shape: sub-ranges of at most 12 A-scans (the model goes bin by bin)"""
    b, a, depth = small.vol.shape
    rng = np.random.default_rng(a)
    cases = []
    for ci, (M, (b0, bn)) in enumerate(small.combos[:3]):
        a0, an, G = small.groups[ci % len(small.groups)]
        if an > 12:
            a0, an = a0 + 1, 12
            G = (1, 4, 12)[ci % 3]
        s0, sn = ((0, depth), (3, depth - 6), (1, depth - 3))[ci % 3]
        region = (b0, bn, a0, an, s0, sn)
        est = rm.repeat_shifts(small.vol, region, M, G, RVOL)[0]
        cases.append((region, M, G, est, _crafted_shifts(rng, bn // M, M, an // G, sn)))
    return cases


def test_registered_volume(small):
    pipe, vol, dvol = small.pipe, small.vol, small.dvol
    k = 0
    seen = set()
    for region, M, G, est, crafted in _registered_cases(small):
        b0, bn, a0, an, s0, sn = region
        mean_all = small.registered(region, M, 0, est, G)
        finite = mean_all[1][mean_all[2] & np.isfinite(mean_all[1])]
        contained = float(np.sort(finite)[finite.size // 2])  # a mean the data contains: bins equal to the threshold are masked
        for method, name in METHODS:
            for shifts in (est, crafted):
                for thr, masked in ((None, 0.0), (contained, -0.0), (np.inf, np.nan)):
                    k += 1
                    fill = (np.nan, -3.5, -0.0)[k % 3]
                    want, want_mean = small.expected(region, M, method, shifts, G, fill, thr, masked)
                    what = (region, M, G, name, thr, "estimated" if shifts is est else "crafted")
                    with_mean, how = divmod((k // 3) % 6, 3)  # (every pairing of mean, memory and mask setting comes up)
                    with_mean = bool(with_mean)
                    seen.add((with_mean, how, thr is None))
                    kw = dict(threshold=thr, masked=masked, ascans_per_group=G, uncovered=fill, **_kw(region))
                    if how == 0:    # shifts from a numpy array, host source and result
                        got = pipe.angiogram(M, name, mean=with_mean, data=vol, shifts=shifts, **kw)
                        got = got if with_mean else (got,)
                    else:           # shifts from a CUDA tensor -- the one register_repeats just wrote, no synchronise in between
                        if how == 2 and shifts is est:
                            dsh = torch.zeros(est.shape, dtype=torch.int32, device="cuda")
                            torch.cuda.synchronize()
                            pipe.register_repeats(M, G, RVOL, data=dvol, out=dsh, **_kw(region))
                        else:
                            dsh = torch.from_numpy(shifts).cuda()
                        pad, out = _guarded(want.shape)
                        mpad, mean = _guarded(want.shape)
                        res = pipe.angiogram(M, name, mean=mean if with_mean else False, data=dvol, out=out, shifts=dsh, **kw)
                        got = tuple(_host(pipe, t) for t in (res if with_mean else (res,)))
                        _guards_intact(pad, what)
                        _guards_intact(mpad, what)
                        if not with_mean:
                            assert np.all(mpad.cpu().numpy() == MARK), ("mean written without mean=", what)
                        if how == 2 and shifts is est:
                            _same(dsh.cpu().numpy(), est, ("chained shifts",) + what)
                    _same(got[0], want, ("contrast",) + what)
                    if with_mean:
                        _same(got[1], want_mean, ("mean",) + what)
    assert len(seen) == 12
    _same(_host(pipe, dvol), vol, "the source volume")


def test_registered_volume_results_off_a_16_byte_boundary(small):
    """results that start 1, 2 and 3 floats past a 16-byte boundary (every row has a head, the mean's alignment differs from the contrast's)"""
    pipe, dvol = small.pipe, small.dvol
    region, M, G, est, crafted = _registered_cases(small)[0]
    want, want_mean = small.expected(region, M, 2, crafted, G, -1.25)
    dsh = torch.from_numpy(crafted).cuda()
    for skew, mean_skew in ((1, 3), (2, 2), (3, 0)):
        pad, mpad = torch.full((want.size + 16,), MARK, device="cuda"), torch.full((want.size + 16,), MARK, device="cuda")
        torch.cuda.synchronize()
        out, mean = pad[4 + skew:4 + skew + want.size].view(want.shape), mpad[mean_skew:mean_skew + want.size].view(want.shape)
        pipe.angiogram(M, "difference", mean=mean, data=dvol, out=out, shifts=dsh, ascans_per_group=G, uncovered=-1.25, **_kw(region))
        _same(_host(pipe, out), want, ("skewed result", skew))
        _same(mean.cpu().numpy(), want_mean, ("skewed mean", mean_skew))
        hp, hm = pad.cpu().numpy(), mpad.cpu().numpy()
        assert np.all(hp[:4 + skew] == MARK) and np.all(hp[4 + skew + want.size:] == MARK), skew
        assert np.all(hm[:mean_skew] == MARK) and np.all(hm[mean_skew + want.size:] == MARK), mean_skew


# ---------------------------------------------------------------------------------------------------------------------- 3. the registered en face
def test_registered_enface(small):
    pipe, vol, dvol = small.pipe, small.vol, small.dvol
    depth = vol.shape[2]
    rng = np.random.default_rng(17)
    k = 0
    for region, M, G, est, crafted in _registered_cases(small):
        b0, bn, a0, an, s0, sn = region
        surface = rng.integers(0, depth, (bn, an)).astype(np.int32)
        surface[rng.random((bn, an)) < 0.25] = -2
        dsurf = torch.from_numpy(surface).cuda()
        for shifts in (est, crafted):
            dsh = torch.from_numpy(shifts).cuda()
            k += 1
            method, name = METHODS[k % 3]
            thr, masked = ((None, 0.0), (0.1, np.nan), (-0.3, -0.0))[k % 3]
            volume = small.expected(region, M, method, shifts, G, MARK, thr, masked)[0]
            # thickness 1, 16, 64, 65, the whole window and more (thicker than Wc), slabs clipped at either end and wholly outside
            slabs = ((0, 1), (-2, 16), (-40, 64), (-30, 65), (-depth, 2 * depth + 1), (3, 4096), (depth + 5, 3), (-depth - 200, 64))
            for i, (offset, thickness) in enumerate(slabs):
                for fn, fname in ((0, "average"), (1, "mip")):
                    fill = np.nan if (i + fn) & 1 else -1.5
                    for given, model_surface in ((dsurf, surface), (None, None), (surface, surface)):
                        if given is not dsurf and (i + k) % 3:
                            continue
                        want = rm.project_registered(volume, region, M, shifts, G, model_surface, offset, thickness, fn, fill)
                        what = (region, M, G, name, thr, offset, thickness, fname, "no surface" if given is None else type(given).__name__)
                        ekw = dict(offset=offset, thickness=thickness, function=fname, fill=fill, threshold=thr, masked=masked,
                                   ascans_per_group=G, **_kw(region))
                        if given is surface:  # everything from the host
                            _same(pipe.angiogram_enface(M, name, surface=given, data=vol, shifts=shifts, **ekw), want, ("en face host",) + what)
                            continue
                        pad, out = _guarded(want.shape)
                        assert pipe.angiogram_enface(M, name, surface=given, data=dvol, out=out, shifts=dsh, **ekw) is out
                        _same(_host(pipe, out), want, ("en face device",) + what)
                        _guards_intact(pad, what)
                        for form in (1, 2) if thickness <= 64 else (1,):  # one wave per A-scan; teams of 16 lanes
                            pad, out = _guarded(want.shape)
                            got, ms = pipe.angiogram_enface_timed(M, name, surface=given, data=dvol, out=out, shifts=dsh, form=form, **ekw)
                            assert got is out and ms > 0.0
                            _same(_host(pipe, out), want, ("en face device, form %d" % form,) + what)
                            _guards_intact(pad, what)
        # one setting straight from the values
        want = rm.angiogram_enface_registered(vol, region, M, 1, crafted, G, surface, -3, 20, 0, -1.0, -0.2, 0.5)
        got = pipe.angiogram_enface(M, "decorrelation", -0.2, 0.5, surface, -3, 20, "average", -1.0, data=dvol, shifts=crafted, ascans_per_group=G,
                                    **_kw(region))
        _same(got, want, ("en face from the values", region))
    _same(_host(pipe, dvol), vol, "the source volume")


# ---------------------------------------------------------------------------------------------------------------------- 4. against the unregistered calls
def test_zero_shifts_give_the_bits_of_the_unregistered_calls_and_huge_shifts_the_fill(small):
    pipe, vol, dvol = small.pipe, small.vol, small.dvol
    b, a, depth = vol.shape
    for ci, (M, (b0, bn)) in enumerate(small.combos):
        a0, an, G = small.groups[ci % len(small.groups)]
        region = (b0, bn, a0, an) + ((0, depth), (3, depth - 6), (2, depth - 5))[ci % 3]
        P, Qp = bn // M, an // G
        zero = np.zeros((P, M, Qp), np.int32)
        dzero = torch.from_numpy(zero).cuda()
        method, name = METHODS[ci % 3]
        kw = dict(threshold=0.0, masked=np.nan, **_kw(region))
        plain = pipe.angiogram(M, name, mean=True, data=dvol, **kw)
        got = pipe.angiogram(M, name, mean=True, data=dvol, shifts=zero, ascans_per_group=G, uncovered=5.0, **kw)
        _same(got[0], plain[0], ("zero shifts", region, M))
        _same(got[1], plain[1], ("zero shifts, mean", region, M))
        for offset, thickness, fn in ((2, 16, "average"), (-3, 64, "mip"), (0, 65, "average"), (0, 4096, "mip")):
            ekw = dict(offset=offset, thickness=thickness, function=fn, fill=-1.0, data=dvol, **kw)
            want = pipe.angiogram_enface(M, name, **ekw)
            _same(pipe.angiogram_enface(M, name, shifts=dzero, ascans_per_group=G, **ekw), want, ("zero shifts, en face", region, M, thickness))
            for form in (1, 2) if thickness <= 64 else (1,):
                _same(pipe.angiogram_enface_timed(M, name, shifts=zero, ascans_per_group=G, form=form, **ekw)[0], want, ("zero shifts", form))
        # shifts larger than the window: nothing is covered, whatever their sign
        for d0, d1 in ((0, region[5]), (0, -region[5]), (-2 ** 31, 2 ** 31 - 1), (region[5], -1)):
            huge = zero.copy()
            huge[:, 0], huge[:, M - 1] = d0, d1
            out, mean = pipe.angiogram(M, name, mean=True, data=dvol, shifts=huge, ascans_per_group=G, uncovered=-0.0, **kw)
            assert np.all(out.view(np.uint32) == 0x80000000) and np.all(mean.view(np.uint32) == 0x80000000), (d0, d1)
            img = pipe.angiogram_enface(M, name, thickness=4096, fill=7.0, data=dvol, shifts=huge, ascans_per_group=G, **kw)
            assert np.all(img == 7.0), (d0, d1)


# ---------------------------------------------------------------------------------------------------------------------- 5. the product
def test_register_then_angiogram_enface_on_the_handles_own_slot_without_a_synchronise():
    n, a, b, M, G, R = 1024, 32, 8, 4, 8, 8
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    devs = [_dev(synthetic_raw(n, a, b, seed=70 + k)) for k in range(2)]
    region = (0, b, 4, 24, 9, 300)
    kw = _kw(region)
    P, Qp = b // M, 24 // G
    pipe.process_device(devs[0].data_ptr())
    first = pipe.register_repeats(M, G, R, **kw)
    pipe.process_device(devs[1].data_ptr())
    # estimate -> registered en face (and volume), everything on the device, no synchronise since process_device
    dsh = torch.zeros((P, M, Qp), dtype=torch.int32, device="cuda")
    dcost = torch.zeros((P, M - 1, Qp, 2 * R + 1), dtype=torch.float64, device="cuda")
    dimg = torch.zeros((P, 24), dtype=torch.float32, device="cuda")
    dvol_out = torch.zeros((P, 24, 300), dtype=torch.float32, device="cuda")
    dsurf = torch.full((b, 24), 40, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pipe.process_device(devs[1].data_ptr())
    pipe.register_repeats(M, G, R, costs=dcost, out=dsh, **kw)
    assert pipe.angiogram_enface(M, "difference", surface=dsurf, offset=2, thickness=16, fill=-1.0, out=dimg, shifts=dsh, ascans_per_group=G, **kw) is dimg
    pipe.angiogram(M, "variance", out=dvol_out, shifts=dsh, ascans_per_group=G, uncovered=-1.0, **kw)
    pipe.synchronize()
    host = pipe.processed_host().reshape(b, a, n // 2).copy()
    want, want_costs, _ = rm.repeat_shifts(host, region, M, G, R)
    _same(dsh.cpu().numpy(), want, "shifts behind process_device")
    _same(dcost.cpu().numpy(), want_costs, "costs behind process_device")
    surface = np.full((b, 24), 40, np.int32)
    _same(dimg.cpu().numpy(), rm.angiogram_enface_registered(host, region, M, am.DIFFERENCE, want, G, surface, 2, 16, 0, -1.0), "chained en face")
    # (the first three A-scans of the region, all of group 0, as a region of one group of three)
    _same(dvol_out.cpu().numpy()[:, :3], rm.angiogram_registered(host, (0, b, 4, 3, 9, 300), M, am.VARIANCE, want[:, :, :1], 3, -1.0)[0], "chained volume")
    # the same bits from the caller's copy in either memory, and from a repeated call
    for what, got in (("repeat", pipe.register_repeats(M, G, R, **kw)), ("host", pipe.register_repeats(M, G, R, data=host, **kw)),
                      ("device", pipe.register_repeats(M, G, R, data=torch.from_numpy(host).cuda(), **kw))):
        _same(got, want, what)
    assert first.shape == want.shape
    # nothing the chain reads or writes was touched: the next buffer is what a fresh handle computes
    pipe.process_device(devs[0].data_ptr())
    pipe.synchronize()
    fresh = Pipeline(v180_benchmark_params(n, a, b), device=0)
    for d in (devs[0], devs[1], devs[1], devs[0]):
        fresh.process_device(d.data_ptr())
    fresh.synchronize()
    assert np.array_equal(pipe.processed_host().view(np.uint32), fresh.processed_host().view(np.uint32))
    fresh.close()
    pipe.close()


def test_registered_plain_and_estimate_calls_take_turns_on_one_handles_scratch():
    """the five calls share one scratch (staged rows, results on their way to the host): a registered volume, a plain en face of another
    shape, a shift estimate and the registered volume again on one handle, everything from and to the host, every result the model's bits"""
    n, a, b = 256, 8, 8
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    vol = np.random.default_rng(41).standard_normal((b, a, n // 2)).astype(np.float32)
    full, part = (0, b, 0, a, 0, n // 2), (0, b, 2, 5, 3, 61)
    shifts = np.random.default_rng(42).integers(-5, 6, (b // 2, 2, a // 4)).astype(np.int32)
    shifts[:, 0] = 0
    shifts[0, 1] = (3, -4)
    surface = np.random.default_rng(43).integers(0, 60, (b, 5)).astype(np.int32)

    def registered():
        return pipe.angiogram(2, "decorrelation", mean=True, data=vol, shifts=shifts, ascans_per_group=4, uncovered=-2.0, **_kw(full))

    want = rm.angiogram_registered(vol, full, 2, am.DECORRELATION, shifts, 4, -2.0)
    first = registered()
    _same(first[0], want[0], "registered contrast")
    _same(first[1], want[1], "registered mean")
    img = pipe.angiogram_enface(4, "variance", surface=surface, offset=1, thickness=5, function="average", fill=-1.0, data=vol, **_kw(part))
    _same(img, am.angiogram_enface(vol, part, 4, am.VARIANCE, surface, 1, 5, 0, -1.0), "plain en face behind a registered volume")
    est, costs = pipe.register_repeats(2, 8, 8, costs=True, data=vol, **_kw(full))
    want_est, want_costs, _ = rm.repeat_shifts(vol, full, 2, 8, 8)
    _same(est, want_est, "shifts behind the en face")
    _same(costs, want_costs, "costs behind the en face")
    again = registered()
    _same(again[0], want[0], "registered contrast, again")
    _same(again[1], want[1], "registered mean, again")
    _same(again[0], first[0], "the repeated call")
    _same(again[1], first[1], "the repeated call's mean")
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 6. errors
def test_argument_errors_and_callbacks():
    n, a, b = 1024, 32, 6
    p = v180_benchmark_params(n, a, b)
    pipe = Pipeline(p, device=0)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=1))
    pipe.synchronize()
    L, h = _lib.lib(), pipe.handle
    outf = np.zeros(b * a * (n // 2), np.float32)
    shifts = np.zeros(b * a, np.int32)
    fp, sp = C.c_void_p(outf.ctypes.data), C.c_void_p(shifts.ctypes.data)
    S, E, G, T = _lib.AngioSettings, _lib.SurfaceEnfaceSettings, _lib.AngioRegistration, _lib.RepeatShiftSettings
    ok = _lib.StatsRegion(0xFFFFFFFF, 0, b, 0, a, 0, n // 2)

    def estimate(reg=ok, repeats=2, g=a, R=8):
        return L.octpipe_repeat_shifts(h, None, 0, C.byref(reg), C.byref(T(repeats, g, R)), sp, 0, None)

    def volume(reg=ok, repeats=2, g=a, sh=sp):
        return L.octpipe_angiogram_registered(h, None, 0, C.byref(reg), C.byref(S(repeats, 0, 0, 0.0, 0.0)), fp, None, 0, sh, 0, C.byref(G(g, 0.0)))

    def enface(reg=ok, repeats=2, g=a, sh=sp, thickness=4):
        return L.octpipe_angiogram_enface_registered(h, None, 0, C.byref(reg), C.byref(S(repeats, 0, 0, 0.0, 0.0)), None, 0,
                                                     C.byref(E(0, thickness, 0, 0.0)), fp, 0, sh, 0, C.byref(G(g, 0.0)))

    def refused(rc, field, code=1):
        assert rc == code and field in L.octpipe_last_error(), (rc, field, L.octpipe_last_error())

    for call in (estimate, volume, enface):
        assert call() == 0 and call(repeats=3) == 0 and call(repeats=6, g=1) == 0 and call(g=16) == 0
        refused(call(repeats=4), b"repeats")  # does not divide the 6 B-scans
        refused(call(repeats=1), b"repeats")
        refused(call(repeats=9), b"repeats")
        refused(call(g=0), b"ascansPerGroup")
        refused(call(g=5), b"ascansPerGroup")
        for reg, field in ((_lib.StatsRegion(0xFFFFFFFF, 0, 0, 0, a, 0, 40), b"bscan"), (_lib.StatsRegion(0xFFFFFFFF, 2, b, 0, a, 0, 40), b"bscan"),
                           (_lib.StatsRegion(0xFFFFFFFF, 0, 2, 1, a, 0, 40), b"Ascan"), (_lib.StatsRegion(0xFFFFFFFF, 0, 2, 0, a, n // 2, 40), b"Sample"),
                           (_lib.StatsRegion(1, 0, 2, 0, a, 0, 40), b"buffer")):
            refused(call(reg), field)
    assert estimate(R=1) == 0 and estimate(R=64) == 0 and estimate(_lib.StatsRegion(0xFFFFFFFF, 0, b, 0, a, 5, 17)) == 0
    refused(estimate(R=0), b"maxShift")
    refused(estimate(R=65), b"maxShift")
    refused(estimate(_lib.StatsRegion(0xFFFFFFFF, 0, b, 0, a, 5, 16)), b"sampleCount")
    refused(volume(sh=None), b"shifts")
    refused(enface(sh=None), b"shifts")
    refused(enface(thickness=0), b"thickness")
    with pytest.raises(OctPipeError, match="repeats"):
        pipe.register_repeats(4)
    with pytest.raises(OctPipeError, match="maxShift"):
        pipe.register_repeats(2, max_shift=65)
    with pytest.raises(ValueError):
        pipe.angiogram(2, shifts=np.zeros(5, np.int32))  # not [P][M][Qp]
    # inside a pipeline callback
    codes = []
    p.streamFloatToHost = 1
    S2 = p.samplesPerBuffer // 2
    fb = [np.zeros(S2, np.float32), np.zeros(S2, np.float32)]
    pipe.register_float_streaming_buffers(fb[0], fb[1])

    def cb(*args):
        codes.extend([estimate(), volume(), enface()])
    pipe.set_callbacks(on_float_streaming=cb)
    pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=3))
    pipe.synchronize()
    assert len(codes) >= 3 and set(codes) == {7}, codes
    pipe.close()
