"""The crafted peak analysis cases (tests/peak_cases.py) on the model alone: every case reaches the branch it declares, and together
they reach every branch of steps 1 to 5 of the definition (include/octpipe.h "peak analysis").  tests/test_gpu_peak_crafted.py holds
the device against the model on exactly these cases; a fixture that drifted off its branch would make that test vacuous."""
import math

import numpy as np
import pytest

import peak_cases as pc
import peak_model as pm

FLOATS = ("value", "position", "left", "right", "fwhm", "amplitude", "center", "sigma", "offset", "fitFwhm", "rms")
INTS = ("index", "fitFirst", "fitCount", "iterations", "status")


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


_MODEL = {}


def _model(case):
    if case.name not in _MODEL:
        _MODEL[case.name] = case.model()
    return _MODEL[case.name]


def _interior_d(case, avg, o, ij):
    """(k strictly inside the window, d of step 3) of a group with a peak"""
    m = avg[ij].astype(np.float64)
    k = o["index"] - case.s0
    if not 0 < k < len(m) - 1:
        return False, None
    return True, (m[k - 1] - 2.0 * m[k]) + m[k + 1]


@pytest.mark.parametrize("case", pc.cases(), ids=lambda c: c.name)
def test_case_reaches_its_branch(case):
    avg, res = _model(case)
    nb, na, ns = case.region.shape
    assert avg.shape == (nb, na // case.g, ns)
    assert np.array_equal(case._cut(case.embed()).view(np.uint32), case.region.view(np.uint32))
    if case.whole is None:
        outside = np.ones(case.embed().shape, bool)
        case._cut(outside)[...] = False
        assert np.all(np.isnan(case.embed()[outside]))
    o = res[case.at[0]][case.at[1]]
    e = dict(case.expect)
    assert (o["status"] & e.pop("has", 0)) == case.expect.get("has", 0), (o["status"], case.expect)
    assert not o["status"] & e.pop("lacks", 0), (o["status"], case.expect)
    if e.pop("auto_width", False):
        assert case.settings["fit_half_width"] == 0 and math.isfinite(o["fwhm"])
        w = int(min(float(pc.CAP_W), max(float(pc.FLOOR_W), math.ceil(1.5 * o["fwhm"]))))
        k = o["index"] - case.s0
        cut = e.pop("cut", None)
        assert (k - w < 0) == (cut == "left") and (k + w > ns - 1) == (cut == "right"), (k, w, cut)
        assert o["fitFirst"] == case.s0 + max(0, k - w) and o["fitCount"] == min(ns - 1, k + w) - max(0, k - w) + 1
        if e.get("fitCount") == 2 * pc.FLOOR_W + 1:
            assert math.ceil(1.5 * o["fwhm"]) < pc.FLOOR_W
        if e.get("fitCount") == 2 * pc.CAP_W + 1:
            assert math.ceil(1.5 * o["fwhm"]) > pc.CAP_W
    reach = e.pop("flank_at_least", None)
    if reach is not None:
        assert o["index"] - o["left"] > reach and o["right"] - o["index"] > reach, (o["left"], o["index"], o["right"])
    bits = e.pop("averaged_bits", None)
    if bits is not None:
        assert np.all(avg.view(np.uint32) == bits)
    for f, want in e.items():
        assert f in FLOATS or f in INTS, f
        if f in FLOATS:
            assert _same(o[f], want), (f, o[f], want)
        else:
            assert o[f] == want, (f, o[f], want)
    if case.nonfinite is not None:
        flagged = {(i, j) for i, row in enumerate(res) for j, r in enumerate(row) if r["status"] & pm.NONFINITE}
        assert flagged == case.nonfinite
    if case.fit_exact:
        assert o["iterations"] == 0 and o["status"] & pm.FIT_CONVERGED  # (no solve runs: nothing is rounded differently)
    if case.fit_close:
        steps = pc.fit_steps(case, case.at)
        assert len(steps) == case.settings["max_iterations"] == o["iterations"] and o["status"] & pm.FIT_MAX_ITER
        for i, s in enumerate(steps):
            print("%s: solve %d %s, cost %.6g -> %s, relative step %s" % (case.name, i + 1, "accepted" if s[0] else "rejected", s[1], s[2], s[3]))
            assert pc.step_is_decisive(s, first=(i == 0)), (i, s)


def test_the_order_of_addition_shows_in_the_chunked_averages():
    """G > 64: the chunked sum differs from the plain sequential one in at least one bit of the averaged A-scans (a kernel that summed
    the rows straight through would not pass), and a last chunk taken as 64 rows would read the next group"""
    for case in pc.cases():
        if not case.name.startswith("average_G") or case.g <= 65:
            continue  # (G = 65: a last chunk of one row, the two orders are the same sum)
        avg, _ = _model(case)
        rows = case.region[0, :case.g].astype(np.float64)
        plain = (pm.seq_sum(rows, axis=0) / np.float64(case.g)).astype(np.float32)
        assert not np.array_equal(plain.view(np.uint32), avg[0, 0].view(np.uint32)), case.name
        assert case.g % pm.CHUNK != 0


def test_cases_cover_every_branch():
    status_or = 0
    seen = set()
    for case in pc.cases():
        avg, res = _model(case)
        ns = case.region.shape[2]
        for i, row in enumerate(res):
            for j, o in enumerate(row):
                st = o["status"]
                status_or |= st
                if st & (pm.NONFINITE | pm.NO_PEAK):
                    continue
                inside, d = _interior_d(case, avg, o, (i, j))
                if inside and d < 0.0:
                    seen.add("d<0")
                    if o["position"] != o["index"]:
                        seen.add("vertex off the sample")
                if not inside:
                    assert o["position"] == o["index"]
                    seen.add("position=k")
                if not st & pm.WIDTH_UNDEFINED:
                    seen.add("left open" if st & pm.LEFT_OPEN else "l>s0")
                    seen.add("right open" if st & pm.RIGHT_OPEN else "r<s1")
                if case.settings["fit"]:
                    if o["fitCount"] < 5:
                        seen.add("fitCount<5")
                    if o["fitCount"] == ns:
                        seen.add("fitCount=window")
                    if o["status"] & pm.FIT_CONVERGED and o["iterations"] == 0:
                        seen.add("C=0 at once")
    for bit in (pm.NO_PEAK, pm.NONFINITE, pm.WIDTH_UNDEFINED, pm.LEFT_OPEN, pm.RIGHT_OPEN, pm.FIT_CONVERGED, pm.FIT_MAX_ITER, pm.FIT_SKIPPED):
        assert status_or & bit, bit
    assert seen == {"d<0", "vertex off the sample", "position=k", "left open", "l>s0", "right open", "r<s1", "fitCount<5", "fitCount=window",
                    "C=0 at once"}, seen
    # the shapes that take another path in the kernels and the launch
    gs = {c.g for c in pc.cases()}
    assert {1, 3, 8, 63, 64, 65, 100, 130, 200} <= gs
    windows = {c.region.shape[2] for c in pc.cases()}
    assert {3, 4, 5, 63, 64, 65, 1024, 1025, 4096} <= windows
    qs = {c.region.shape[0] * c.region.shape[1] // c.g for c in pc.cases()}
    assert {1, 2, 3, 5} <= qs
    assert {c.s0 % 4 == 0 for c in pc.cases()} == {True, False}


def test_max_iteration_fixture_is_the_documented_one():
    y = pc.max_iteration_fixture()
    assert y.shape == (200,) and y.dtype == np.float32
    for it in (1, 2, 3):
        o = pm.analyse(y, fit=True, max_iterations=it)
        assert o["status"] & pm.FIT_MAX_ITER and o["iterations"] == it
