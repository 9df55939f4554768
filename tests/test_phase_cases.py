"""The case tables of tests/phase_cases.py, proved on the model alone: every instance and launch shape of the accumulate kernel is
reached (through accumulate_form, the restatement of launchAccumulate), every extraction case makes the lane scans and the clamps work,
and the float32-transform model stays within a quarter of the bound the device is held to.  Plus the host staging arithmetic of
csrc/phase_stage.h under the address and undefined-behaviour sanitizers (tests/native/phase_stage_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import phase_cases as pc
import phase_model as pm

CURVE_ATOL = 1e-3  # samples: tests/test_gpu_phase_extraction.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------- accumulate
def _launches():
    return [(c, l) for c in pc.ACCUMULATE_CASES for l in c.launches()]


def test_encode_round_trips_and_packs_across_rows():
    rng = np.random.default_rng(1)
    for fmt, bd in pc.FORMATS:
        for n in (8, 9):
            ints = pc._random_ints(rng, (4, n), fmt, bd)
            raw, dec = pc._encode(ints, fmt, bd)
            if fmt in (1, 2):  # (the random draw is the 12-bit pattern)
                assert np.array_equal(dec & 0xFFF, ints) and dec.min() >= (0 if fmt == 1 else -2048) and dec.max() <= (4095 if fmt == 1 else 2047)
                flat = raw.reshape(-1)
                assert flat.size == 4 * n * 3 // 2
                got = np.array([pc.decode_packed(flat, i, fmt == 2) for i in range(4 * n)]).reshape(4, n)
                assert np.array_equal(got, dec)
            else:
                assert np.array_equal(dec, ints)
            lo, hi = pc.value_range(fmt, bd)
            ex = pc._extreme_ints(rng, (64, n), fmt, bd)
            assert set(np.unique(ex)) == {lo, hi} and np.array_equal(pc._encode(ex, fmt, bd)[1], ex)


def test_accumulate_form_restates_the_launch_rule():
    # (vec, chunks, rowsPerPass, colBlocks)
    assert pc.accumulate_form(0, 12, 1024, 0, False) == (True, 128, 2, 1)
    assert pc.accumulate_form(0, 12, 1024, 2, False) == (False, 1024, 1, 4)
    assert pc.accumulate_form(0, 12, 1024, 2, True) == (True, 128, 2, 1)  # staged: aligned
    assert pc.accumulate_form(0, 12, 1000, 0, False) == (True, 125, 2, 1) and pc.accumulate_form(0, 12, 1664, 0, True)[0]
    assert pc.accumulate_form(0, 12, 130, 0, True) == (False, 130, 1, 1)
    assert pc.accumulate_form(0, 12, 96, 2, False) == (False, 96, 2, 1)
    assert pc.accumulate_form(0, 8, 96, 0, True) == (True, 6, 42, 1)
    assert pc.accumulate_form(0, 8, 256, 0, False) == (True, 16, 16, 1)
    assert pc.accumulate_form(0, 32, 1024, 0, False) == (True, 256, 1, 1)
    assert pc.accumulate_form(0, 32, 2048, 0, False) == (True, 512, 1, 2)
    assert pc.accumulate_form(1, 12, 1024, 4, False) == (True, 128, 2, 1) and pc.accumulate_form(1, 12, 1024, 3, False) == (False, 1024, 1, 4)
    assert pc.accumulate_form(2, 12, 129, 0, True) == (False, 129, 1, 1)


def test_every_format_runs_in_both_forms():
    seen = {(c.fmt, min(c.bit_depth, 12) if c.fmt == 0 and c.bit_depth in (12, 16) else c.bit_depth, l[0]) for c, l in _launches()}
    assert seen == {(f, b, v) for f, b in pc.FORMATS for v in (True, False)}
    # ... and the extremes of every format in both forms, the twin handle's launches included
    for fmt, bd in pc.FORMATS:
        forms = set()
        for c in pc.ACCUMULATE_CASES:
            if c.values == "extremes" and c.fmt == fmt:
                forms |= {c.form(s)[0] for _, _, s in c.calls + c.twin_calls()}
        assert forms == {True, False}, (fmt, bd)
    for c in pc.ACCUMULATE_CASES:
        if c.source == "sliced":
            assert c.offset == {0: 3, 1: 1, 2: 2, 4: 4}[pc.elem_bytes(c.fmt, c.bit_depth)] and not c.form()[0]


def test_the_launch_shapes_the_issue_lists():
    L = _launches()

    def has(pred):
        return [c.name for c, l in L if pred(c, *l)]

    # the vector form in more than one column block: uint16 at 4096, uint32 and int32 at 2048
    wide = {(c.fmt, c.n) for c, (vec, rpp, cb, rg, fr, rows) in L if vec and cb > 1}
    assert {(0, 4096), (0, 2048), (5, 2048)} <= wide
    # the scalar form in more than one column block with a partial last one; N = 130 as one partial block
    assert has(lambda c, vec, rpp, cb, rg, fr, rows: not vec and cb > 1 and c.n % pc.THREADS != 0 and c.n == 1000)
    assert has(lambda c, vec, rpp, cb, rg, fr, rows: not vec and cb == 1 and rpp == 1 and c.n == 130)
    # the scalar form with rowsPerPass = 2 and idle threads (rowOff >= rowsPerPass)
    assert has(lambda c, vec, rpp, cb, rg, fr, rows: not vec and rpp == 2 and pc.THREADS % c.form()[1] != 0 and c.n == 96)
    # the vector form with rowsPerPass 2, 4 and 16; and with idle threads
    for want in (2, 4, 16):
        assert has(lambda c, vec, rpp, cb, rg, fr, rows: vec and rpp == want), want
    assert has(lambda c, vec, rpp, cb, rg, fr, rows: vec and rpp == 42)
    # ascanCount 1, 2, 3, 5; a count below rowsPerPass; the whole buffer; a device firstRow that is odd and no multiple of rowsPerPass
    for want in (1, 2, 3, 5):
        assert has(lambda c, vec, rpp, cb, rg, fr, rows: rows == want), want
    assert has(lambda c, vec, rpp, cb, rg, fr, rows: rpp > 1 and rows < rpp)
    assert has(lambda c, vec, rpp, cb, rg, fr, rows: rpp > 2 and fr % 2 == 1 and fr % rpp != 0)
    assert all(any(f == 0 and n == c.lines for f, n, _ in c.calls) for c in pc.ACCUMULATE_CASES)
    # more than one row group, and behind the unrolled loop a tail of 1, 2 and 3 rows (37 rows with rowsPerPass = 1: 9 groups)
    assert pc.row_groups(37, 1, 1) == 9 and sorted(set(pc.lane_row_counts(37, 1, 9))) == [4, 5]
    # (rowGroups = passes / 4 keeps a lane below 7 rows as soon as there are two groups: the tail of 3 comes from 7 rows in one group)
    tails, left = set(), set()
    for c, (vec, rpp, cb, rg, fr, rows) in L:
        if rg > 1:
            left.add((vec, rows % (pc.UNROLL * rg * rpp)))
        for k in pc.lane_row_counts(rows, rpp, rg):
            if k >= pc.UNROLL:
                tails.add((vec, rg > 1, k % pc.UNROLL))
    assert {(v, t) for v in (True, False) for t in (1, 2, 3)} <= left, left
    assert {(v, True, t) for v in (True, False) for t in (1, 2)} | {(v, False, 3) for v in (True, False)} <= tails, tails
    # two sources into one accumulator
    assert sum(len({s for _, _, s in c.calls}) > 1 for c in pc.ACCUMULATE_CASES) >= 4
    # a case per format under each bitshift
    assert {(c.fmt, c.bit_depth, c.bitshift) for c in pc.ACCUMULATE_CASES} >= {(f, b, s) for f, b in pc.FORMATS for s in (0, 1)}
    assert all(c.lines <= 600 for c in pc.ACCUMULATE_CASES)
    # lengths: powers of two apart from the four the suite already builds handles for
    assert {c.n for c in pc.ACCUMULATE_CASES if c.n & (c.n - 1)} == {96, 130, 1000}


def test_twin_calls_cover_the_same_rows_from_the_other_memory():
    for c in pc.ACCUMULATE_CASES:
        _, dec = c.data()
        twin = c.twin_calls()
        a, b = c.expected(dec), c.expected(dec, twin)
        assert a[1] == b[1] and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), c.name
        assert len(twin) <= len(c.calls) and {s for _, _, s in twin} != {s for _, _, s in c.calls}, c.name
    assert sum(len(c.twin_calls()) < len(c.calls) for c in pc.ACCUMULATE_CASES) >= 16  # one call instead of several
    # the constant rows: dropping or repeating one row changes the mean's bits
    c = [c for c in pc.ACCUMULATE_CASES if c.values == "rows"][0]
    _, dec = c.data()
    want = c.expected(dec)[0]
    wrong = c.expected(dec, c.calls[:-1] + [(c.calls[-1][0] + 1, c.calls[-1][1], "device")])[0]
    assert not np.array_equal(want, wrong)


def test_packed_odd_rows_and_the_defect_they_showed():
    """N = 129, firstAscan = 1: the row starts in byte 192 on the odd sample of its pair; offset firstAscan * floor(1.5 N) = 193 (the
    host path's arithmetic before csrc/phase_stage.h) decodes other samples"""
    for fmt, n, a, b in pc.PACKED_ODD:
        for source in ("host", "device"):
            c = pc.packed_odd_case(fmt, n, a, b, source)
            assert not c.form()[0] and (n * a * b) % 2 == 0
            assert {f for f, _, _ in c.calls} == {0, 1, 2, 3} and (0, a * b, source) in c.calls
            raw, dec = c.data()
            assert raw.ndim == 1 and raw.size == n * a * b * 3 // 2
    c = pc.packed_odd_case(1, 129, 4, 2, "host")
    raw, dec = c.data()
    assert (1 * 129) >> 1 == 64 and 64 * 3 == 192 and (3 * 129) // 2 == 193
    stale = pc.stale_host_rows(raw, 129, 1, 1)
    old = np.array([pc.decode_packed(np.concatenate([stale, [0, 0]]), i, False) for i in range(129)])
    assert not np.array_equal(old, dec[1])
    # what the fixed path stages: from the even row below, the kernel skipping one row
    staged = raw[0:(2 * 129 * 3 + 1) // 2]
    new = np.array([pc.decode_packed(staged, 129 + i, False) for i in range(129)])
    assert np.array_equal(new, dec[1])
    # a whole-buffer call copied lines / 2 bytes too few
    assert 8 * 193 == raw.size - 4


def test_staging_arithmetic_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "phase_stage_check")
    src = os.path.join(ROOT, "tests", "native", "phase_stage_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "all checks passed" in out.stdout


# ---------------------------------------------------------------------------------------------------------------------- extract
def test_two_tone_mean():
    m = pc.two_tone_mean(256, 3, 8, 0.95)
    j = np.arange(256)
    want = 2048 + 600 * np.cos(2 * np.pi * 3 * j / 256) + 0.95 * 600 * np.cos(2 * np.pi * 8 * j / 256 + 0.7)
    assert m.dtype == np.float32 and np.array_equal(m, want.astype(np.float32))
    X = np.abs(np.fft.fft(m.astype(np.float64)))
    assert sorted(np.argsort(X[1:128])[-2:] + 1) == [3, 8]


@pytest.mark.parametrize("case", pc.EXTRACT_CASES, ids=repr)
def test_extract_case_reaches_the_scans_and_clamps(case):
    n, a, b = case.n, case.a, case.b
    p = n // 64
    w = case.model()
    mono = w["psi_mono"]
    assert np.all(np.diff(mono) >= 0) and (w["a"], w["b"]) == (a, b)
    runs = pc.changed_runs(w, n)
    if case.name.startswith("tones"):
        # a run of changed samples over 3 or more lane segments needs the exclusive scan of the lane totals: the middle lane gets its
        # level from a lane that is not its neighbour.  Asked on each side of the anchor that is 8 or more segments long.
        up = [r for r in runs if r[0] > a and r[2] >= 3]
        down = [r for r in runs if r[1] < a and r[2] >= 3]
        assert (n - 1 - a < 8 * p) or up, runs
        assert (a < 8 * p) or down, runs
        assert up or down
        assert a != n // 2 + 3 or a % p != 0  # off a lane boundary
    else:
        assert all(r[2] < 3 for r in runs)  # the clean fringe: the case is here for the upper clamp
    # entries within CURVE_ATOL of a clamp's border may round to either side on the device: at most 4 per case
    assert int(pc.near_clamp(mono, n, CURVE_ATOL).sum()) <= 4


def test_both_clamps_occur():
    below = {c.name: int((np.arange(c.n) < c.model()["psi_mono"][0]).sum()) for c in pc.EXTRACT_CASES}
    above = {c.name: int((np.arange(c.n) >= c.model()["psi_mono"][-1]).sum()) for c in pc.EXTRACT_CASES}
    print("entries below the first level:", below)
    print("entries at or above the last level:", above)
    for n in pc.LENGTHS:
        assert 26 <= below["tones-3-8-%d" % n] and 26 <= below["tones-4-7-%d" % n] and 26 <= below["tones-3-8-%d-anchor-last-lane" % n]
        assert above["fringe-%d-short-b" % n] >= 2
        c = [c for c in pc.EXTRACT_CASES if c.name == "fringe-%d-short-b" % n][0]
        assert np.count_nonzero(c.model()["curve"] == n - 1) == above[c.name]
    assert below["tones-3-8-256-anchor-0"] == 0  # the anchor is sample 0 and level 0: nothing lies below it


def test_cubic_fit_reference_on_a_short_interval():
    """pm.fit_cubic solves the normal equations in rational arithmetic.  On a wide [a, b] float64 lstsq on the powers of t agrees with
    it; on the 11 samples next to N-1 of the anchor-in-the-last-lane cases it does not (and the float64 normal equations in powers
    of t, the library's fit before it moved to the centred variable, kept no digit there)."""
    for n in (256, 4096):
        for name in ("tones-3-8-%d", "tones-3-8-%d-anchor-last-lane"):
            c = [c for c in pc.EXTRACT_CASES if c.name == name % n][0]
            curve = c.model(np.complex64)["curve"].astype(np.float32)
            exact = pm.fit_cubic(curve, c.a, c.b)
            t = np.arange(c.a, c.b + 1, dtype=np.float64) / (n - 1)
            V = np.stack([np.ones_like(t), t, t * t, t * t * t], axis=1)
            lstsq = np.linalg.lstsq(V, curve.astype(np.float64)[c.a:c.b + 1], rcond=None)[0]
            y = curve.astype(np.float64)[c.a:c.b + 1]
            assert np.linalg.norm(V @ exact - y) <= np.linalg.norm(V @ lstsq - y) * (1 + 1e-6) + 1e-9
            if c.a == n // 2 + 3:
                np.testing.assert_allclose(lstsq, exact, rtol=1e-6, atol=1e-6)
            print(c.name, "cond %.1e" % np.linalg.cond(V), "lstsq - exact", lstsq - exact)


def test_silent_band_is_silent():
    """period 4 in float32: tones at N/4 and N/2 leave every other bin at exactly zero, whatever the order of the sums"""
    for n in pc.LENGTHS:
        c = pc.silent_band_case(n)
        m = c.mean()
        assert np.array_equal(m, np.tile(m[:4], n // 4)) and len(set(m[:4].tolist())) >= 3
        assert c.peak[1] < n // 4 and c.peak[0] >= 2
        with pytest.raises(ValueError):
            c.model()


def test_float32_transforms_stay_within_a_quarter_of_the_bound():
    """The device transforms in float32.  Its curve is held to a forward residual |psi_mono64(curve[j]) - j| <= CURVE_ATOL; the same
    model with complex64 transforms must use no more than a quarter of that.  (The residual, not the curve difference, is bounded: on
    a flat stretch of psi_mono the curve jumps by the stretch's length for an infinitesimal change of level.)"""
    rows = []
    for c in pc.EXTRACT_CASES:
        w64, w32 = c.model(), c.model(np.complex64)
        mono = w64["psi_mono"]
        j = np.arange(c.n, dtype=np.float64)
        d = pc.domain(mono, c.n)
        res = np.abs(pm.forward(mono, w32["curve"]) - j)[d].max()
        res_f32 = np.abs(pm.forward(mono, w32["curve"].astype(np.float32)) - j)[d].max()
        diff = np.abs(w32["curve"] - w64["curve"])[d].max()
        flips = int(((w32["curve"] == 0) != (w64["curve"] == 0)).sum() + ((w32["curve"] == c.n - 1) != (w64["curve"] == c.n - 1)).sum())
        rows.append((c.name, res, res_f32, diff, flips, float(np.diff(mono).max())))
    print("%-34s %-11s %-13s %-11s %s" % ("case", "residual", "as float32", "curve diff", "clamp flips / steepest psi step"))
    for r in rows:
        print("%-34s %.2e    %.2e      %.2e    %d / %.1f" % r)
    for name, res, _, _, flips, _ in rows:
        assert res <= CURVE_ATOL / 4, (name, res)
        assert flips <= 4, (name, flips)
