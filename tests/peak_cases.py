"""Crafted A-scans for the peak analysis (include/octpipe.h "peak analysis"): one case per branch of the definition and per load path
of csrc/peak_analysis.h / csrc/pipe_peak.hip.  tests/test_peak_cases.py proves on the model alone (tests/peak_model.py) that every case
reaches the branch it declares; tests/test_gpu_peak_crafted.py runs exactly these cases on the device.  Seeded generators and literal
arrays only: no device, no files.

A case is a region [bscanCount][ascanCount][sampleCount] of float32 that starts at (first_bscan, first_ascan, s0) of a buffer
[B][A][L], the group size G, the settings, and `expect`: what the model must report for group `at` (status bits that must be set /
clear, index, position, ...).  Case.embed() gives the whole buffer: the case's own (`whole`), or NaN everywhere outside the region, so
that a value read from outside the region and added to a result shows as NONFINITE or in the averaged bits."""
import numpy as np

import peak_model as pm

F32 = np.float32
NAN = F32("nan")
FLOOR_W, CAP_W = 4, 256  # the automatic fit half width's limits (step 5 of the definition)

# the buffers the cases live in, (N, A, B) of the handle: rows of L = N / 2 = 512 values for windows up to 500, of 4096 beyond
SMALL, LARGE = (1024, 416, 3), (8192, 72, 2)


class Case:
    def __init__(self, name, region, g=1, s0=8, handle=SMALL, origin=(1, 3), whole=None, at=(0, 0), expect=None, nonfinite=None,
                 fit_exact=False, fit_close=False, **settings):
        region = np.asarray(region, dtype=F32)
        if region.ndim == 1:
            region = region[None, None, :]
        self.name, self.region, self.g, self.s0, self.handle, self.origin = name, region, int(g), int(s0), handle, origin
        self.whole = whole          # the whole buffer [B][A][L], or None: NaN outside the region
        self.at = at                # the group `expect` speaks of
        self.expect = expect or {}  # has / lacks (status bits), index, value, position, left, right, fwhm, fitFirst, fitCount, ...
        self.nonfinite = nonfinite  # None, or the set of groups (i, j) that are NONFINITE: exactly those
        self.fit_exact = fit_exact  # every fit field is bit-equal between model and device (no iteration runs)
        self.fit_close = fit_close  # the fit's end state does not hang on rounding: parameters are compared
        self.settings = dict(threshold=-np.inf, fit=False, fit_half_width=0, max_iterations=0)
        self.settings.update(settings)
        n, a, b = handle
        nb, na, ns = region.shape
        assert na % self.g == 0 and 3 <= ns <= 4096
        assert origin[0] + nb <= b and origin[1] + na <= a and self.s0 + ns <= n // 2, name
        if whole is not None:
            assert whole.shape == (b, a, n // 2) and whole.dtype == F32
            assert np.array_equal(self._cut(whole).view(np.uint32), region.view(np.uint32)), name

    def _cut(self, buf):
        (fb, fa), (nb, na, ns) = self.origin, self.region.shape
        return buf[fb:fb + nb, fa:fa + na, self.s0:self.s0 + ns]

    def embed(self):
        """the whole buffer [B][A][L] (a fresh array)"""
        if self.whole is not None:
            return self.whole.copy()
        n, a, b = self.handle
        buf = np.full((b, a, n // 2), NAN, F32)
        self._cut(buf)[...] = self.region
        return buf

    def region_args(self):
        """bscans, ascans, depth, ascans_per_group of Pipeline.peak_analysis"""
        (fb, fa), (nb, na, ns) = self.origin, self.region.shape
        return dict(bscans=(fb, nb), ascans=(fa, na), depth=(self.s0, ns), ascans_per_group=self.g)

    def model(self, **over):
        """(averaged, per-group dicts) of tests/peak_model.py with the case's settings (over: settings to replace)"""
        kw = dict(self.settings)
        kw.update(over)
        with np.errstate(invalid="ignore"):  # (+inf and -inf meet in a sum on purpose)
            return pm.analyse_region(self.region, self.g, s0=self.s0, **kw)


def f32(x):
    return np.asarray(x, dtype=F32)


def floor_noise(seed, n, top=1.0):
    """n values in [0, top): the floor the crafted samples are put on"""
    return (np.random.default_rng(seed).random(n) * top).astype(F32)


def gaussian(n, mu, sigma, amp=100.0, offset=1.0, noise=0.0, seed=0):
    z = np.arange(n, dtype=np.float64)
    y = amp * np.exp(-0.5 * ((z - mu) / sigma) ** 2) + offset
    if noise:
        y = y + np.random.default_rng(seed).normal(0.0, noise, n)
    return y.astype(F32)


def spread_rows(seed, shape, g):
    """rows whose magnitudes span 10**U(-3, 7), as tests/test_peak_analysis.py::test_chunked_average, and that cancel within each group
    of g: all but one or two of a group's rows come in pairs x, -x, shuffled, and the one or two left over are small.  The float64 sum of
    a group is then the rounding its order of addition leaves plus the small rows, so another order shows in the float32 bits of
    the average, not only in the last bits of the float64 sum"""
    rng = np.random.default_rng(seed)
    b, a, s = shape
    out = np.empty(shape, F32)
    for i in range(b):
        for q in range(a // g):
            h = (g - 1) // 2  # pairs; one or two small rows remain
            big = (rng.standard_normal((h, s)) * 10 ** rng.uniform(-3, 7, size=(h, 1))).astype(F32)
            small = (rng.standard_normal((g - 2 * h, s)) * 10 ** rng.uniform(-3, -1)).astype(F32)
            out[i, q * g:(q + 1) * g] = rng.permutation(np.concatenate([big, -big, small]), axis=0)
    return out


def max_iteration_fixture():
    """200 samples of a noisy Gaussian: with max_iterations 1, 2, 3 the model ends in FIT_MAX_ITER after that many solves"""
    rng = np.random.default_rng(7)
    z = np.arange(200, dtype=np.float64)
    return (100.0 * np.exp(-0.5 * ((z - 90.3) / 6.0) ** 2) + 1.0 + rng.normal(0.0, 2.0, 200)).astype(F32)


def fit_steps(case, at=(0, 0)):
    """the model's Levenberg-Marquardt steps of one group replayed: a list of (accepted, cost before, cost after or None, largest
    relative step or None) for each of the max_iterations solves (the definition's loop, tests/peak_model.marquardt)"""
    avg, res = case.model()
    o, m = res[at[0]][at[1]], avg[at].astype(np.float64)
    lo, cnt = o["fitFirst"] - case.s0, o["fitCount"]
    z, y = np.arange(o["fitFirst"], o["fitFirst"] + cnt, dtype=np.float64), m[lo:lo + cnt]
    c0 = float(y.min())
    p = np.array([o["value"] - c0, o["position"], max(0.5, o["fwhm"] / pm.FWHM_PER_SIGMA), c0])
    H, g, cost = pm._sums(z, y, p)
    lam, steps = 1e-3, []
    for _ in range(case.settings["max_iterations"]):
        d = pm.solve(H, g, lam)
        cn = None if d is None else pm._sums(z, y, p + d)
        if cn is not None and cn[2] < cost:
            steps.append((True, cost, cn[2], float(np.max(np.abs(d) / (np.abs(p) + 1e-12)))))
            p, (H, g, cost), lam = p + d, cn, max(lam / 10.0, 1e-15)
        else:
            steps.append((False, cost, None if cn is None else cn[2], None))
            lam *= 10.0
    return steps


def step_is_decisive(step, first=True):
    """the step's outcome cannot turn on the last bits of the sums.  The first solve: rejected, or accepted with C(p') < 0.99 C(p) and
    a relative step above 1e-6.  A later solve: the decisions of the loop are C(p') < C(p), C(p) - C(p') <= 1e-12 C(p) and a relative
    step <= 1e-10, and two float64 evaluations of sums over some hundred samples differ by some 1e-13 of their value: a cost that
    moves by more than 1e-6 of itself, either way, and a relative step above 1e-6 leave every one of them seven orders of margin."""
    accepted, cost, after, rel = step
    if accepted:
        return after < (0.99 if first else 1.0 - 1e-6) * cost and after != 0.0 and rel > 1e-6
    return after is None or after > (1.0 + 1e-6) * cost


# ------------------------------------------------------------------------------------------------------------------------ the cases
def _argmax():
    out = []

    def with_max(name, n, where, s0=8, **expect):
        m = floor_noise(len(out) + 10, n)
        m[list(where)] = 5.0
        expect.setdefault("index", s0 + min(where))
        expect.setdefault("value", 5.0)
        out.append(Case(name, m, s0=s0, expect=expect))

    with_max("argmax_twice_in_one_lane_3_67", 128, (3, 67), lacks=pm.LEFT_OPEN | pm.RIGHT_OPEN)
    with_max("argmax_later_lane_smaller_index_70_5", 128, (70, 5), s0=9)
    with_max("argmax_plateau_60_70", 128, range(60, 71), position=8 + 60.5)
    with_max("argmax_first_sample", 128, (0,), s0=0, has=pm.LEFT_OPEN, position=0.0, left=0.0)
    with_max("argmax_last_sample", 128, (127,), has=pm.RIGHT_OPEN, position=8 + 127.0, right=8 + 127.0)
    with_max("argmax_sample_64_of_65", 65, (64,), s0=3, has=pm.RIGHT_OPEN)
    for n in (3, 4, 5, 63, 64, 65):
        with_max("window_of_%d" % n, n, (n // 2,), s0=(8 if n % 2 else 5))
    with_max("window_of_63_last", 63, (62,), has=pm.RIGHT_OPEN)
    with_max("window_of_64_last", 64, (63,), has=pm.RIGHT_OPEN)
    # -0.0 before 0.0: equal values, the first wins and its bits are reported
    for name, n, neg, pos in (("negzero_then_zero_adjacent", 6, 1, 2), ("negzero_then_zero_one_lane_3_67", 80, 3, 67),
                              ("negzero_5_zero_70", 80, 5, 70)):
        m = np.full(n, -1.0, F32)
        m[neg], m[pos] = -0.0, 0.0
        out.append(Case(name, m, expect=dict(index=8 + neg, value=-0.0, has=pm.WIDTH_UNDEFINED)))
    return out


def _threshold():
    v = F32(1234.567)
    m = floor_noise(30, 40)
    m[17] = v
    below = float(np.nextafter(v, F32(0)))
    ml, mr = float(m[16]), float(m[18])
    nan = float("nan")
    return [Case("threshold_equal_to_value", m, threshold=float(v), expect=dict(has=pm.NO_PEAK, index=25, value=float(v), position=nan)),
            Case("threshold_equal_to_value_fit_on", m, threshold=float(v), fit=True, expect=dict(has=pm.NO_PEAK, lacks=pm.FIT_BITS, fitCount=0)),
            Case("threshold_one_ulp_below_value", m, threshold=below, expect=dict(lacks=pm.NO_PEAK, index=25, position=25.0 + (0.5 * (ml - mr)) / ((ml - 2.0 * float(v)) + mr))),
            Case("threshold_minus_inf_all_negative", f32([-5, -3, -1, -3, -5]), s0=9,
                 expect=dict(lacks=pm.NO_PEAK, has=pm.WIDTH_UNDEFINED, index=11, value=-1.0, position=11.0))]


def _nonfinite():
    out = []
    for name, bad in (("nan", np.nan), ("plus_inf", np.inf), ("minus_inf", -np.inf)):
        m = floor_noise(40, 100) + F32(1)
        m[37] = bad
        out.append(Case("one_%s_in_the_window" % name, m, expect=dict(has=pm.NONFINITE, index=0), nonfinite={(0, 0)}))
    m = floor_noise(41, 100) + F32(1)
    m[99] = np.nan
    out.append(Case("nan_in_the_last_sample_fit_on", m, fit=True, expect=dict(has=pm.NONFINITE, lacks=pm.FIT_BITS, fitCount=0), nonfinite={(0, 0)}))
    rows = np.stack([floor_noise(42, 90), floor_noise(43, 90)])[None]
    rows[0, 0, 10], rows[0, 1, 10] = np.inf, -np.inf
    out.append(Case("plus_inf_and_minus_inf_average_to_nan", rows, g=2, expect=dict(has=pm.NONFINITE), nonfinite={(0, 0)}))
    # NaN only just outside the window, in every row of an otherwise finite buffer: both load forms (s0 % 4 == 0: 16-byte loads that
    # reach up to 3 values past the window's end; s0 odd: value by value)
    for s0 in (8, 9):
        for g in (1, 8, 130):
            n, a, b = SMALL
            ns = 61
            whole = (np.random.default_rng(50 + s0 + g).random((b, a, n // 2)) + 1.0).astype(F32)
            whole[:, :, s0 - 1] = np.nan
            whole[:, :, s0 + ns] = np.nan
            na = 8 if g < 64 else 260
            out.append(Case("nan_at_s0_minus_1_and_past_the_end_s0_%d_G%d" % (s0, g), whole[1:3, 3:3 + na, s0:s0 + ns], g=g, s0=s0, whole=whole,
                            expect=dict(lacks=pm.NONFINITE), nonfinite=set()))
    # NaN in rows next to a group border (and, G = 130, next to the chunk borders inside a group) flags that group alone
    for g in (8, 130):
        def rows(seed):
            return (np.random.default_rng(seed).random((1, 3 * g, 70)) + 1.0).astype(F32)
        r = rows(60)
        r[0, 2 * g - 1, 11] = np.nan
        out.append(Case("nan_in_the_last_row_of_group_1_G%d" % g, r, g=g, s0=4, nonfinite={(0, 1)}))
        r = rows(61)
        r[0, g, 69] = np.nan
        out.append(Case("nan_in_the_first_row_of_group_1_G%d" % g, r, g=g, s0=5, nonfinite={(0, 1)}))
        r = rows(62)
        r[0, g - 1, 0], r[0, g, 1] = np.nan, np.nan
        out.append(Case("nan_on_both_sides_of_the_border_of_groups_0_and_1_G%d" % g, r, g=g, s0=4, nonfinite={(0, 0), (0, 1)}))
    r = (np.random.default_rng(63).random((1, 390, 70)) + 1.0).astype(F32)
    for k, row in enumerate((63, 64, 127, 128)):
        r[0, 130 + row, 5 + 13 * k] = np.nan
    out.append(Case("nan_in_rows_63_64_127_128_of_group_1_G130", r, g=130, s0=12, nonfinite={(0, 1)}))
    return out


def _parabola():
    return [Case("parabola_peak_on_the_left_edge", f32([9, 4, 1, 0, 0]), s0=7, expect=dict(position=7.0, index=7, has=pm.LEFT_OPEN)),
            Case("parabola_peak_on_the_right_edge", f32([0, 0, 1, 4, 9]), s0=7, expect=dict(position=11.0, index=11, has=pm.RIGHT_OPEN)),
            Case("parabola_equal_neighbour_vertex_halfway", f32([0, 4, 4, 0, 0]), expect=dict(position=9.5, index=9)),
            Case("parabola_asymmetric", f32([0, 1, 7, 10, 4, 0, 0]), s0=1, expect=dict(index=4, position=4.0 + (0.5 * (7.0 - 4.0)) / ((7.0 - 20.0) + 4.0))),
            Case("parabola_near_flt_max", f32([3e38, 3.4e38, 3e38, -3.4e38, 0]), s0=0,
                 expect=dict(index=1, position=1.0, has=pm.LEFT_OPEN, lacks=pm.RIGHT_OPEN | pm.NONFINITE)),
            Case("parabola_near_flt_max_asymmetric", f32([0, 2.5e38, 3.4e38, 3.3e38, 0, 0]), s0=3, expect=dict(index=5, lacks=pm.STEP4_BITS))]


def _width():
    out = [Case("width_all_zero", np.zeros(8, F32), expect=dict(has=pm.WIDTH_UNDEFINED, index=8, value=0.0, position=8.0)),
           Case("width_all_negative_zero", np.full(70, -0.0, F32), s0=5, expect=dict(has=pm.WIDTH_UNDEFINED, index=5, value=-0.0)),
           Case("width_all_negative", -1.0 - floor_noise(70, 70), expect=dict(has=pm.WIDTH_UNDEFINED, lacks=pm.NO_PEAK)),
           Case("width_all_negative_fit_on", -1.0 - 0.01 * (np.arange(60, dtype=F32) - 30) ** 2, fit=True,
                expect=dict(has=pm.WIDTH_UNDEFINED, index=38, fitFirst=22, fitCount=33))]
    # flanks wider than one and two 64-sample ballot blocks on either side
    for name, sigma, reach in (("64", 80.0, 64), ("128", 120.0, 128)):
        m = gaussian(400, 200.3, sigma, amp=10.0, offset=0.0) + F32(0.01) * floor_noise(71, 400)
        out.append(Case("width_flanks_beyond_%s_samples" % name, m, s0=11, expect=dict(lacks=pm.LEFT_OPEN | pm.RIGHT_OPEN, flank_at_least=reach)))
    # the first sample at or below half sits on the last lane of a ballot block (offset 63), the first lane of the next (64), one
    # further (65); a sample above half lies beyond it, which a scan from the wrong end would take
    for off in (63, 64, 65):
        k, n = 100, 200
        jl, jr = k - 1 - off, k + 1 + off
        m = floor_noise(72 + off, n, 3.0)
        m[jl + 1:jr] = 8.0
        m[k] = 10.0
        m[jl], m[jr] = 1.0, 2.0
        m[jl - 1], m[jr + 1] = 9.0, 9.0
        out.append(Case("width_crossings_at_offset_%d" % off, m, s0=4,
                        expect=dict(index=4 + k, left=4 + (jl + 1) - (8.0 - 5.0) / (8.0 - 1.0), right=4 + (jr - 1) + (8.0 - 5.0) / (8.0 - 2.0),
                                    lacks=pm.LEFT_OPEN | pm.RIGHT_OPEN)))
    # a crossing on the window's first / last sample is a crossing; none is an open flank (k = 10: first block; k = 65: lane 0 of the second)
    for k in (10, 65):
        n = k + 1 + k
        m = np.full(n, 8.0, F32)
        m[k] = 10.0
        closed = m.copy()
        closed[0], closed[n - 1] = 1.0, 2.0
        out.append(Case("width_crossings_on_the_first_and_last_sample_k%d" % k, closed, s0=6,
                        expect=dict(lacks=pm.LEFT_OPEN | pm.RIGHT_OPEN, left=6 + 1 - 3.0 / 7.0, right=6 + (n - 2) + 3.0 / 6.0)))
        out.append(Case("width_no_crossing_on_either_side_k%d" % k, m, s0=6,
                        expect=dict(has=pm.LEFT_OPEN | pm.RIGHT_OPEN, left=6.0, right=6.0 + n - 1, fwhm=n - 1.0)))
        half_open = m.copy()
        half_open[0] = 1.0
        out.append(Case("width_right_open_only_k%d" % k, half_open, s0=7, expect=dict(has=pm.RIGHT_OPEN, lacks=pm.LEFT_OPEN)))
        half_open = m.copy()
        half_open[n - 1] = 1.0
        out.append(Case("width_left_open_only_k%d" % k, half_open, s0=7, expect=dict(has=pm.LEFT_OPEN, lacks=pm.RIGHT_OPEN)))
    out.append(Case("width_sample_equal_to_half", f32([0, 7, 4, 6, 8, 4, 7, 0]), s0=2,
                    expect=dict(index=6, left=4.0, right=7.0, fwhm=3.0, lacks=pm.LEFT_OPEN | pm.RIGHT_OPEN)))
    out.append(Case("width_float32_denormals", f32([0, 1e-45, 3e-45, 1e-45, 0, 0]), s0=8,
                    expect=dict(index=10, value=float(F32(3e-45)), position=10.0, left=9.0, right=11.0, fwhm=2.0, lacks=pm.STEP4_BITS)))
    return out


def _averaging():
    out = []
    # G up to 64: one pass; beyond: chunk partials (the last chunk 1, 36, 2 and 8 rows).  300 samples: two stage-A tiles, the second
    # partly filled; group counts 1, 2, 3, 5 and 6 leave waves of the last workgroup idle
    for g, nb, q, s0 in ((1, 1, 5, 8), (3, 1, 3, 9), (8, 1, 5, 8), (63, 2, 1, 7), (64, 1, 1, 8), (64, 1, 2, 5), (65, 1, 3, 8), (100, 2, 2, 9),
                         (130, 1, 3, 8), (200, 1, 2, 6), (200, 2, 2, 8)):
        region = spread_rows(100 + g + q, (nb, g * q, 300), g)
        out.append(Case("average_G%d_Q%d" % (g, nb * q), region, g=g, s0=s0, expect=dict(lacks=pm.NONFINITE), nonfinite=set()))
    for g in (8, 130):
        out.append(Case("average_of_negative_zero_G%d" % g, np.full((1, g, 66), -0.0, F32), g=g,
                        expect=dict(has=pm.WIDTH_UNDEFINED, index=8, value=-0.0, averaged_bits=0x80000000)))
    # 1024 samples: the last window with four waves per workgroup; 1025: the first with one; 4096: the longest
    for ns, s0 in ((1024, 8), (1025, 7), (4096, 0)):
        region = gaussian(ns, ns - 24.6, 5.0, noise=0.5, seed=ns)[None, None, :] + np.random.default_rng(ns + 1).random((1, 15, ns)).astype(F32)
        region[0, 3:6] += gaussian(ns, 30.2, 4.0, amp=300.0, offset=0.0)  # group 1 peaks near the other end
        out.append(Case("window_of_%d_G3_Q5" % ns, region, g=3, s0=s0, handle=LARGE, fit=True, at=(0, 1), expect=dict(index=s0 + 30, lacks=pm.STEP4_BITS | pm.FIT_SKIPPED)))
        out.append(Case("window_of_%d_G65" % ns, spread_rows(ns, (1, 65, ns), 65), g=65, s0=s0, handle=LARGE, origin=(0, 2)))
    return out


def _fit_windows():
    out = []
    y = gaussian(200, 90.3, 6.0, noise=1.0, seed=80)
    k = int(np.argmax(y))
    out.append(Case("fit_half_width_1_skipped", y, fit=True, fit_half_width=1, expect=dict(has=pm.FIT_SKIPPED, fitFirst=8 + k - 1, fitCount=3)))
    edge = gaussian(200, 0.0, 6.0, noise=0.0)
    out.append(Case("fit_half_width_2_peak_on_the_edge_skipped", edge, fit=True, fit_half_width=2, s0=5, expect=dict(has=pm.FIT_SKIPPED, index=5, fitFirst=5, fitCount=3)))
    out.append(Case("fit_half_width_2_peak_on_the_far_edge_skipped", edge[::-1].copy(), fit=True, fit_half_width=2, s0=5, expect=dict(has=pm.FIT_SKIPPED, fitFirst=202, fitCount=3)))
    out.append(Case("fit_half_width_2_inside_five_samples", y, fit=True, fit_half_width=2, expect=dict(lacks=pm.FIT_SKIPPED, fitFirst=8 + k - 2, fitCount=5)))
    out.append(Case("fit_half_width_10", y, fit=True, fit_half_width=10, s0=9, expect=dict(lacks=pm.FIT_SKIPPED, fitFirst=9 + k - 10, fitCount=21)))
    for w in (0xFFFFFFFF, 0xFFFFFF00, 0x80000000):
        out.append(Case("fit_half_width_0x%08X_whole_window" % w, y, fit=True, fit_half_width=w, expect=dict(lacks=pm.FIT_SKIPPED, fitFirst=8, fitCount=200)))
    out.append(Case("fit_half_width_200_is_the_window", y, fit=True, fit_half_width=200, expect=dict(fitFirst=8, fitCount=200)))
    # the automatic width min(256, max(4, ceil(1.5 fwhm))): cut by either edge of the window, at its floor, at its cap
    left = gaussian(200, 6.4, 6.0, noise=0.2, seed=81)
    out.append(Case("fit_auto_width_cut_by_the_left_edge", left, fit=True, expect=dict(fitFirst=8, auto_width=True, cut="left")))
    out.append(Case("fit_auto_width_cut_by_the_right_edge", left[::-1].copy(), fit=True, s0=9, expect=dict(auto_width=True, cut="right")))
    spike = floor_noise(82, 120, 0.5)
    spike[60] = 10.0
    out.append(Case("fit_auto_width_at_its_floor", spike, fit=True, expect=dict(fitFirst=8 + 60 - FLOOR_W, fitCount=2 * FLOOR_W + 1, auto_width=True)))
    wide = gaussian(700, 350.4, 100.0, noise=0.3, seed=83)
    out.append(Case("fit_auto_width_at_its_cap", wide, fit=True, handle=LARGE, s0=16, expect=dict(fitCount=2 * CAP_W + 1, auto_width=True)))
    return out


def _fit_states():
    out = [Case("fit_flat_converged_at_once", np.full(40, 7.25, F32), s0=5, fit=True, fit_exact=True,
                expect=dict(status=pm.LEFT_OPEN | pm.RIGHT_OPEN | pm.FIT_CONVERGED, iterations=0, amplitude=0.0, offset=7.25, center=5.0, rms=0.0,
                            sigma=39.0 / pm.FWHM_PER_SIGMA, fitFwhm=39.00000000000001, fitFirst=5, fitCount=40))]
    # (the third solve lowers the cost by 7e-7 of itself: accepted, but below the margin step_is_decisive asks for, so its parameters
    # are not compared; status and iterations are)
    y = max_iteration_fixture()
    for it in (1, 2, 3):
        out.append(Case("fit_max_iterations_%d" % it, y, fit=True, max_iterations=it, fit_close=it < 3, expect=dict(has=pm.FIT_MAX_ITER, iterations=it)))
    return out


_CASES = None


def cases():
    """every case, in a fixed order (built once: the arrays are shared and must not be written to)"""
    global _CASES
    if _CASES is None:
        _CASES = _argmax() + _threshold() + _nonfinite() + _parabola() + _width() + _averaging() + _fit_windows() + _fit_states()
        names = [c.name for c in _CASES]
        assert len(set(names)) == len(names)
        for c in _CASES:
            c.region.setflags(write=False)
    return _CASES
