"""The crafted image statistics cases (tests/stats_cases.py) on the model and the restated host arithmetic alone: every case reaches the
path it declares.  tests/test_gpu_stats_crafted.py holds the device against the model on exactly these cases; a fixture that drifted
off its path would make that test vacuous.

a) more segments than workgroups, for both caps; b) at least two staging slices with a border strictly inside a B-scan; c) the vector
form with sampleCount % V != 0; d) wave instructions that are uniform with every lane active, uniform with lane 0 among the inactive
ones, and split by exactly one lane; e) values whose uncorrected reciprocal quotient is not the bin; f) a float64 yardstick that agrees
with exact arithmetic to 1e-12 on the moment cases."""
import numpy as np
import pytest

import stats_cases as sc
import stats_model as sm


def _outside_is_poison(case, whole):
    (fb, nb), (fa, na), (s0, cnt) = case.bscans, case.ascans, case.window
    out = np.ones(whole.shape, bool)
    out[fb:fb + nb, fa:fa + na, s0:s0 + cnt] = False
    if not out.any():
        return None
    o = whole[out]
    if case.fmt == sc.F32:
        assert np.all(np.isnan(o)), case.name
        return np.nan
    assert np.all(o == o[0]), case.name
    return int(sm.decoded(np.int64(o[0]), case.fmt[0], case.fmt[1], case.bitshift))


def _check_poison_shows(case, whole):
    """the poison is beyond every value of the region and outside every explicit range of the case"""
    p = _outside_is_poison(case, whole)
    if p is None or case.fmt == sc.F32:
        return
    v = case.values(whole)
    assert p > v.max() or p < v.min(), (case.name, p)
    for bins, rng in case.runs:
        if rng is not None:
            assert sc.raw_bins([p], bins, *rng)[0] == -1, (case.name, bins, rng)


# ---------------------------------------------------------------------------------------------------------------- the restatement itself
def test_lane_map_is_the_item_order_of_the_header():
    """lane t takes items t, t + 256, ...; item il is values il % G * V .. of row il // G: spelled out thread by thread"""
    plan = sc.Plan(sc.F32, (1024, 32, 4), (1, 2), (3, 7), (4, 203))
    assert (plan.V, plan.G, plan.rows, plan.seg_rows, plan.segments) == (4, 51, 14, 5, 3)
    cnt = 203
    maps = plan.lane_map()
    assert len(maps) == 3
    seen = np.zeros(plan.rows * cnt, int)
    for seg, m in enumerate(maps):
        items = min(5, plan.rows - 5 * seg) * plan.G
        for il in range(m.shape[0] * 64):
            t = il % 256
            for j in range(4):
                got = m[il // 64, j, t % 64]
                s = il % plan.G * 4 + j
                if il < items and s < cnt:
                    assert got == (5 * seg + il // plan.G) * cnt + s
                    seen[got] += 1
                else:
                    assert got == -1
    assert np.all(seen == 1)


def test_packed_window_decode_is_the_model_decode():
    rng = np.random.default_rng(1)
    for fmt in ((1, 12), (2, 12)):
        ints = sm.random_ints(rng, (3, 5, 1001 * 2), fmt[0], 12)
        raw, dec = sm.encode(ints, fmt[0], 12)
        rows = np.array([0, 3, 7, 14])
        got = sc.decode_packed_window(raw, fmt, 1001 * 2, rows, (7, 61))
        assert np.array_equal(got, dec.reshape(15, -1)[rows, 7:68])
    raw = rng.integers(0, 256, size=1001 * 6 * 3 // 2, dtype=np.uint8)
    want = sm.encode(np.zeros(1001 * 6, np.int64), 1, 12)[0]  # (shape only: the bytes of six odd rows)
    assert want.size == raw.size
    v = sc.decode_packed_window(raw, (1, 12), 1001, np.arange(6), (0, 1001)).ravel()
    assert np.array_equal(sm.encode(v, 1, 12)[0], raw)  # any byte string is valid packed data, and the decode inverts the encode


# ---------------------------------------------------------------------------------------------------------------- c) load forms
@pytest.mark.parametrize("fmt", sc.LOAD_FORMATS, ids=lambda f: sc.FORMAT_ID[f])
def test_load_form_cases_take_their_form(fmt):
    tails = 0
    for bitshift in ((0, 1) if sc.has_bitshift(fmt) else (0,)):
        cases = sc.load_form_cases(fmt, bitshift)
        assert len(cases) == 36
        for case in cases:
            p = case.plan
            assert p.L % p.V == 0
            assert p.vector_form(0) == case.expect["vector"] and p.vector_form(staged=True) == case.expect["vector"], case.name
            for off in sc.load_offsets(fmt):
                assert not p.vector_form(off), (case.name, off)
            tails += case.expect["vector"] and case.window[1] % p.V != 0
            whole = case.whole()
            _check_poison_shows(case, whole)
            if case.window[1] > 5 * p.V:  # the full rows: the explicit range has values on both sides
                bins, rng = case.runs[0]
                want = case.model(case.values(whole), bins, rng)
                assert want["underflow"] > 0 and want["overflow"] > 0 and np.count_nonzero(want["histogram"]) > bins // 2, case.name
        if fmt != sc.F32 and not sc.packed(fmt):
            assert all(o % sc.ELEM_BYTES[fmt] == 0 or sc.ELEM_BYTES[fmt] == 1 for o in sc.load_offsets(fmt))
    assert tails >= 9  # V - 1, V + 1 and 2V + 3 values at each of the three aligned starts


# ---------------------------------------------------------------------------------------------------------------- a) segment grid
_GRID = {}


def _grid_whole(case):
    if case.fmt not in _GRID:
        _GRID[case.fmt] = case.whole()
    return _GRID[case.fmt]


@pytest.mark.parametrize("case", sc.grid_cases(), ids=repr)
def test_grid_cases_have_more_segments_than_workgroups(case):
    p, e = case.plan, case.expect
    bins = case.runs[0][0]
    assert (p.G, p.seg_rows, p.segments) == (e["G"], e["seg_rows"], e["segments"])
    cap = p.group_cap(bins)
    assert cap == (1024 if bins > 512 else 2048) and p.groups(bins) == e["groups"]
    if bins == 512:
        assert p.segments < cap and p.groups(bins) == p.segments  # the control: still under the wide cap
    else:
        assert p.segments > cap  # some workgroup takes a second segment
    whole = _grid_whole(case)
    assert whole.nbytes // (2 if case.fmt == sc.F32 else 8) <= 9_100_000  # (float32 4 bytes; the raw integers are int64 here, 1 byte on the device)
    v = case.values(whole)
    want = case.model(v, *case.runs[0])
    if case.fmt == sc.F32:  # the B-scan no region reaches is poison
        assert np.all(np.isnan(whole[-1]))
        assert want["underflow"] > 0 and want["overflow"] > 0 and want["nonFinite"] > 0 and want["histogram"].min() > 0
    else:
        # the poison is above every value (max); 256 bins end below it and below the top values (overflow), more bins hold every value
        poison = sc.POISON[case.fmt]
        assert np.all(whole[-1] == poison) and v.min() == 0 and v.max() == 254 < poison
        assert want["histogram"][poison + 40:].sum() == 0
        assert (want["overflow"] > 0) == (bins == 256) and np.count_nonzero(want["histogram"]) == min(bins, 255 + 40) - 40
    assert int(want["histogram"].sum()) + want["underflow"] + want["overflow"] == want["count"] == v.size - want["nonFinite"]


def test_both_caps_are_exceeded():
    caps = {c.plan.group_cap(c.runs[0][0]) for c in sc.grid_cases() if c.plan.segments > c.plan.group_cap(c.runs[0][0])}
    assert caps == {1024, 2048}


# ---------------------------------------------------------------------------------------------------------------- b) staging slices
@pytest.mark.parametrize("case", sc.slice_cases(), ids=repr)
def test_slice_cases_are_staged_in_slices(case):
    p, e = case.plan, case.expect
    na = case.ascans[1]
    assert p.seg_rows == e["seg_rows"] and p.slice_segments() == e["slice_segments"] and p.slice_borders() == e["borders"]
    assert len(p.slice_borders()) + 1 >= 2
    assert any(r % na != 0 for r in p.slice_borders())  # a border strictly inside a B-scan
    assert p.slice_segments() < p.segments
    if sc.packed(case.fmt):
        assert p.parity() and not p.vector_form(staged=True) and case.window[0] % 2 == 1
        assert p.slice_borders()[0] % na == e["border_in_bscan"]
        assert p.segments == -(-p.rows // 32) and p.slice_segments() == 1390
        n, a, b = case.handle
        assert 73 << 20 <= n * a * b * 3 // 2 <= 74 << 20
    else:
        assert p.vector_form(staged=True) and case.window[1] % p.V != 0
    assert (p.rows * (p.row_bytes() + 3)) > sc.STAGE_BYTES


# ---------------------------------------------------------------------------------------------------------------- d) wave-uniform add
@pytest.mark.parametrize("case", sc.wave_cases(), ids=repr)
def test_wave_cases_hold_every_kind_of_wave_instruction(case):
    p = case.plan
    assert p.vector_form(0) and case.window[1] % p.V != 0 and p.G % 64 != 0 and p.segments > 1
    whole = case.whole()
    _check_poison_shows(case, whole)
    v = case.values(whole)
    assert [b for b, _ in case.runs] == list(sc.WAVE_BINS)
    for bins, rng in case.runs:
        b = case.bins_of(v, bins, rng)
        want = case.model(v, bins, rng)
        assert np.array_equal(np.bincount(b[b >= 0], minlength=bins), want["histogram"].astype(np.int64))
        assert want["underflow"] > 0 and want["overflow"] > 0
        c = sc.wave_census(p, b)
        print(case.name, bins, c)
        assert c["full"] >= 50 and c["lane0_off"] >= 5 and c["partial"] > c["lane0_off"] and c["idle"] >= 10, (bins, c)
        if bins > 1:
            assert c["one_off"] >= 3 and c["mixed"] >= 3, (bins, c)  # (one bin: a value is in it or in no bin, no wave is split)
    if case.fmt == sc.F32:
        assert case.model(v, 8, case.runs[2][1])["nonFinite"] > 0


# ---------------------------------------------------------------------------------------------------------------- e) binning edges
@pytest.mark.parametrize("case", sc.raw_edge_cases(), ids=repr)
def test_raw_edge_cases_need_the_correction(case):
    whole = case.whole()
    v = case.values(whole).ravel()
    for bins, rng in case.runs:
        want = case.model(v, bins, rng)
        if rng is None:
            assert want["binWidth"] == -(-2 ** 32 // bins) and want["min"] == sc.LIMITS[case.fmt][0] and want["max"] == sc.LIMITS[case.fmt][1]
            continue
        lo, width = rng
        inr = np.unique(v[sc.raw_bins(v, bins, lo, width) >= 0])
        off = [int(x) for x in inr if sc.uncorrected_bin(int(x) - lo, width) != (int(x) - lo) // width]
        assert all(sc.uncorrected_bin(x - lo, width) == (x - lo) // width - 1 for x in off)  # never too large: only q++ can run
        if case.expect["corrected"]:
            assert off, case.name
            assert want["underflow"] > 0 or lo <= sc.LIMITS[case.fmt][0]
        if width == sc.CONTROL_WIDTH:
            assert not off


def test_the_correction_is_needed_where_the_survey_found_it():
    for width in sc.CORRECTED_WIDTHS:
        assert any(sc.uncorrected_bin(m * width, width) == m - 1 for m in range(1, 4096)), width
    for width in (3, 7, 1000, sc.CONTROL_WIDTH):
        assert all(sc.uncorrected_bin(m * width, width) == m for m in range(4096)), width


@pytest.mark.parametrize("case", sc.processed_edge_cases(), ids=repr)
def test_processed_edge_cases(case):
    v = case.values(case.whole())
    for bins, rng in case.runs:
        want = case.model(v, bins, rng)
        if rng is None:
            assert want["underflow"] == want["overflow"] == 0 and int(want["histogram"].sum()) == v.size
            lo, hi = np.float32(want["lo"]), np.float32(want["hi"])
            assert np.nextafter(lo, np.float32(np.inf)) == hi
            if bins == 1 or float(sm.processed_scale(bins, lo, hi)) == sm.FLT_MAX:
                assert want["histogram"][0] == v.size  # (the clamped scale leaves both floats in bin 0: the definition's answer)
            else:
                assert want["histogram"][0] == np.count_nonzero(v == lo) > 0 and want["histogram"][-1] == np.count_nonzero(v == hi) > 0
            continue
        lo, hi = np.float32(rng[0]), np.float32(rng[1])
        scale = sm.processed_scale(bins, lo, hi)
        if case.expect.get("clamps"):
            assert float(scale) == sm.FLT_MAX and float(bins) / (float(hi) - float(lo)) > sm.FLT_MAX
            assert np.any((v != 0) & (np.abs(v) < np.float32(1.1754944e-38)))  # subnormal values
        if case.expect.get("overflows"):
            inr = v[(v >= lo) & (v <= hi)]
            with np.errstate(over="ignore"):
                t = (inr - lo).astype(np.float32)
            assert np.isinf(t).any() and np.all(sc.processed_bins(inr[np.isinf(t)], bins, lo, hi) == bins - 1)
        assert want["underflow"] > 0 and want["overflow"] > 0 and want["histogram"].sum() > 0


# ---------------------------------------------------------------------------------------------------------------- f) moments
def _naive_std(x):
    x = np.asarray(x, np.float64)
    return float(np.sqrt(max(0.0, float(np.mean(x * x)) - float(np.mean(x)) ** 2)))


@pytest.mark.parametrize("case", sc.moment_cases(), ids=repr)
def test_moment_yardstick_is_exact_to_1e_12(case):
    whole = case.whole()
    _check_poison_shows(case, whole)
    v = case.values(whole)
    want = case.model(v, *case.runs[0])
    mean, std = sc.exact_moments(v)
    scale = max(abs(mean), std)
    assert abs(want["mean"] - mean) <= 1e-12 * scale, (want["mean"], mean)
    assert abs(want["stddev"] - std) <= 1e-12 * std or want["stddev"] == std == 0.0, (want["stddev"], std)
    kind = case.expect["kind"]
    if kind in ("2^23+U64", "1e30-ulps", "-1e-30-ulps", "u32-top", "i32-bottom"):
        assert abs(_naive_std(v) - std) > 1e-8 * std  # what the shift K and the float64 merges are for


def test_sub_regions_of_both_handles_hold_the_same_values():
    cases = sc.moment_cases()
    for i in range(0, len(cases), 3):
        whole32, sub32, sub48 = cases[i:i + 3]
        assert not whole32.expect["sub"] and sub32.expect["sub"] and sub48.expect["sub"]
        assert sub32.handle[1] == 32 and sub48.handle[1] == 48
        assert (sub32.bscans, sub32.ascans, sub32.window) == (sub48.bscans, sub48.ascans, sub48.window)
        a, b = sub32.values(sub32.whole()), sub48.values(sub48.whole())
        assert a.tobytes() == b.tobytes()
        assert (sub32.plan.seg_rows, sub32.plan.segments) == (sub48.plan.seg_rows, sub48.plan.segments)
