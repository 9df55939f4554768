"""Crafted regions for the image statistics (include/octpipe.h "image statistics"): one family of cases per path of csrc/image_stats.h,
csrc/pipe_stats.hip and the staging of csrc/pipe_region.hip that random data at small shapes never takes.  tests/test_stats_cases.py
proves on the model alone (tests/stats_model.py) and on the restated host arithmetic below that every case reaches the path it declares;
tests/test_gpu_stats_crafted.py runs exactly these cases on the device.  Seeded generators and literal values only: no device, no files.

A case names the handle (N, A, B), the sample format and bitshift, the region, the (bins, range) pairs it is run with, a generator of
the whole buffer, and the path it is for.  Outside the region the buffer is poisoned, so that a value read from outside shows in a
count: processed buffers hold NaN there (nonFinite), raw buffers POISON[fmt], a value beyond every explicit range a case uses and beyond
every value of the region (overflow and max; the cases whose values sit at the top of the container poison with its lowest value:
underflow and min).

Plan restates the host arithmetic of csrc/pipe_stats.hip that decides the path: V, G, segRows, segments (validate), the workgroup cap
(groupCap), the load form (launch) and the staging slices (pass).  Plan.lane_map() is the item-to-lane map of the header comment of
csrc/image_stats.h: lane t of a workgroup takes items t, t + 256, ... of a segment, so one wave instruction covers the items
64q .. 64q + 63 of a segment at one value index j."""
import numpy as np

import stats_model as sm

F32 = "f32"  # the processed source; the raw containers are the (format, bitDepth) pairs of stats_model.FORMATS
NAN = np.float32("nan")

# csrc/image_stats.h, csrc/pipe_stats.hip
THREADS, SEG_VALUES, SEG_TARGET = 256, 32768, 2048
MAX_GROUPS, MAX_GROUPS_WIDE, STAGE_BYTES = 2048, 1024, 64 << 20
# csrc/sample_decode.h: values per vector load, bytes per element (packed 12 bit: 3 bytes per pair)
VECTOR = {F32: 4, (0, 8): 16, (0, 12): 8, (0, 32): 4, (1, 12): 8, (2, 12): 8, (3, 8): 16, (4, 16): 8, (5, 32): 4}
ELEM_BYTES = {F32: 4, (0, 8): 1, (0, 12): 2, (0, 32): 4, (3, 8): 1, (4, 16): 2, (5, 32): 4}
# the stored integers a container holds, and the poison outside a raw region (the top of the container)
LIMITS = {(0, 8): (0, 255), (0, 12): (0, 65535), (0, 32): (0, 2 ** 32 - 1), (1, 12): (0, 4095), (2, 12): (-2048, 2047),
          (3, 8): (-128, 127), (4, 16): (-32768, 32767), (5, 32): (-2 ** 31, 2 ** 31 - 1)}
POISON = {f: hi for f, (lo, hi) in LIMITS.items()}
FORMAT_ID = dict(zip(sm.FORMATS, sm.FORMAT_IDS))
FORMAT_ID[F32] = "f32"


def packed(fmt):
    return fmt != F32 and fmt[0] in (1, 2)


class Plan:
    """what csrc/pipe_stats.hip derives from a region's shape"""

    def __init__(self, fmt, handle, bscans, ascans, window):
        self.fmt, self.handle, self.bscans, self.ascans, self.window = fmt, handle, bscans, ascans, window
        self.N, self.A, self.B = handle
        self.L = self.N // 2 if fmt == F32 else self.N
        (fb, nb), (fa, na), (s0, cnt) = bscans, ascans, window
        assert nb >= 1 and na >= 1 and cnt >= 1 and fb + nb <= self.B and fa + na <= self.A and s0 + cnt <= self.L
        self.V = VECTOR[fmt]
        self.G = -(-cnt // self.V)
        self.rows = nb * na
        items = self.rows * self.G
        seg_items = min(SEG_VALUES // self.V, max(THREADS, -(-items // SEG_TARGET)))
        self.seg_rows = max(1, seg_items // self.G)
        self.segments = -(-self.rows // self.seg_rows)

    def group_cap(self, bins):
        values = self.rows * self.window[1]
        return max(MAX_GROUPS_WIDE if bins > 512 else MAX_GROUPS, (values >> 31) + 1)

    def groups(self, bins, segments=None):
        return min(self.segments if segments is None else segments, self.group_cap(bins))

    def parity(self):
        """a staged copy of packed rows of odd length keeps each B-scan run on its own sample parity"""
        return packed(self.fmt) and self.N % 2 == 1

    def vector_form(self, base=0, staged=False):
        """base: the address of element 0 (only its low bits matter); staged: a host source (the staging buffer is aligned)"""
        if staged:
            if self.parity():
                return False
            base = 0
        return self.L % self.V == 0 and self.window[0] % self.V == 0 and base % (4 if packed(self.fmt) else 16) == 0

    def row_bytes(self):
        return (self.L + 1) // 2 * 3 if packed(self.fmt) else self.L * ELEM_BYTES[self.fmt]

    def slice_segments(self):
        return max(1, STAGE_BYTES // ((self.row_bytes() + 3) * self.seg_rows + 64))

    def slice_borders(self):
        """the region rows at which a host source's next staging slice begins"""
        step = self.slice_segments() * self.seg_rows
        return list(range(step, self.rows, step))

    def lane_map(self):
        """per segment an int array [q][j][lane]: the index row * sampleCount + s (region row, sample of the window) of the value lane
        `lane` has at value index j in the wave instruction that covers items 64q .. 64q + 63; -1 where the lane has none"""
        cnt = self.window[1]
        out = []
        for seg in range(self.segments):
            row0 = seg * self.seg_rows
            items = min(self.seg_rows, self.rows - row0) * self.G
            il = np.arange(-(-items // 64) * 64)
            rr, k = il // self.G, il % self.G
            s = k[:, None] * self.V + np.arange(self.V)[None, :]
            idx = (row0 + rr)[:, None] * cnt + s
            idx[(il >= items)[:, None] | (s >= cnt)] = -1
            out.append(idx.reshape(-1, 64, self.V).transpose(0, 2, 1))
        return out


def wave_census(plan, bin_of):
    """bin_of: the bin of every value of the region in (row, sample) order, -1 for a value that enters no bin.  The wave instructions of
    the histogram by what csrc/image_stats.h `count` does with them: idle (no active lane), full (one bin, 64 active lanes), partial
    (one bin, fewer), lane0_off (partial, lane 0 inactive), one_off (two bins, one of them in a single lane), mixed (anything else)"""
    c = dict(idle=0, full=0, partial=0, lane0_off=0, one_off=0, mixed=0)
    bin_of = np.asarray(bin_of).ravel()
    for m in plan.lane_map():
        b = np.where(m >= 0, bin_of[np.maximum(m, 0)], -1).reshape(-1, 64)
        act = b >= 0
        n = act.sum(axis=1)
        b0 = b[np.arange(len(b)), act.argmax(axis=1)]
        same = ((b == b0[:, None]) & act).sum(axis=1)
        uniform = (n > 0) & (same == n)
        c["idle"] += int((n == 0).sum())
        c["full"] += int((uniform & (n == 64)).sum())
        c["partial"] += int((uniform & (n < 64)).sum())
        c["lane0_off"] += int((uniform & (n < 64) & ~act[:, 0]).sum())
        for i in np.flatnonzero((n > 0) & ~uniform):
            counts = np.unique(b[i][act[i]], return_counts=True)[1]
            c["one_off" if len(counts) == 2 and counts.min() == 1 and n[i] >= 3 else "mixed"] += 1
    return c


def processed_bins(values, bins, lo, hi):
    """the bin of each float32 value as include/octpipe.h defines it (tests/stats_model.processed), -1: not finite or out of range"""
    v = np.asarray(values, np.float32).ravel()
    lo, hi = np.float32(lo), np.float32(hi)
    ok = np.isfinite(v) & (v >= lo) & (v <= hi)
    with np.errstate(over="ignore", invalid="ignore"):
        fl = np.floor((v - lo).astype(np.float32) * sm.processed_scale(bins, lo, hi))
    return np.where(ok, np.where(fl >= bins - 1, bins - 1, np.where(ok, fl, 0)), -1).astype(np.int64)


def raw_bins(values, bins, lo, width):
    x = np.asarray(values, np.int64).ravel()
    d = (x - int(lo)) // int(width)
    return np.where((x >= lo) & (d < bins), d, -1)


def decode_packed_window(raw, fmt, n, rows, window):
    """the samples [s0, s0 + cnt) of the buffer rows `rows` of packed 12-bit bytes (rows of n samples), decoded (before bitshift)"""
    s0, cnt = window
    e = np.asarray(rows, np.int64)[:, None] * n + s0 + np.arange(cnt)[None, :]
    b = (e >> 1) * 3
    b0, b1, b2 = raw[b].astype(np.int64), raw[b + 1].astype(np.int64), raw[b + 2].astype(np.int64)
    v = np.where(e & 1, (b1 >> 4) | (b2 << 4), b0 | ((b1 & 15) << 8))
    return v if fmt[0] == 1 else (v ^ 0x800) - 0x800


class Case:
    """make(): the whole buffer -- float32 [B][A][L] (processed), the stored integers [B][A][N] as int64 (raw), or with as_bytes the
    raw bytes themselves (packed 12 bit, flat uint8).  runs: the (bins, range) pairs, range None (autoRange), (lo, hi) (processed)
    or (lo, binWidth) (raw)."""

    def __init__(self, name, path, handle, fmt, bscans, ascans, window, make, runs, bitshift=0, as_bytes=False, expect=None):
        self.name, self.path, self.handle, self.fmt, self.bitshift = name, path, handle, fmt, int(bitshift)
        self.bscans, self.ascans, self.window = bscans, ascans, window
        self.plan = Plan(fmt, handle, bscans, ascans, window)
        self.make, self.runs, self.as_bytes = make, list(runs), as_bytes
        self.expect = expect or {}

    def whole(self):
        w = self.make()
        n, a, b = self.handle
        if self.as_bytes:
            assert w.dtype == np.uint8 and w.size == b * a * n * 3 // 2
        elif self.fmt == F32:
            assert w.dtype == np.float32 and w.shape == (b, a, n // 2)
        else:
            lo, hi = LIMITS[self.fmt]
            assert w.shape == (b, a, n) and w.min() >= lo and w.max() <= hi, self.name
        return w

    def source(self, whole):
        """what the product is given: the float32 buffer, or the raw bytes (flat uint8)"""
        if self.fmt == F32 or self.as_bytes:
            return whole
        return np.ascontiguousarray(sm.encode(whole, *self.fmt)[0])

    def region_rows(self):
        """the buffer rows of the region's rows, in region order"""
        (fb, nb), (fa, na) = self.bscans, self.ascans
        return ((fb + np.arange(nb))[:, None] * self.handle[1] + fa + np.arange(na)[None, :]).ravel()

    def values(self, whole):
        """the region's values as the statistics see them, [rows][sampleCount]: float32, or int64 after decode and bitshift"""
        s0, cnt = self.window
        if self.as_bytes:
            v = decode_packed_window(whole, self.fmt, self.handle[0], self.region_rows(), self.window)
        else:
            v = sm.region_of(whole, self.bscans, self.ascans, self.window).reshape(-1, cnt)
        if self.fmt == F32:
            return v
        if not self.as_bytes:
            v = sm.encode(v, *self.fmt)[1]
        return sm.decoded(v, self.fmt[0], self.fmt[1], self.bitshift)

    def model(self, values, bins, rng):
        f = sm.processed if self.fmt == F32 else sm.raw
        return f(values, bins, *(rng or (None, None)))

    def bins_of(self, values, bins, rng):
        """the bin of every value under an explicit range (wave_census)"""
        return (processed_bins if self.fmt == F32 else raw_bins)(values, bins, *rng)

    def call_args(self, bins, rng):
        """keyword arguments of Pipeline.processed_statistics / raw_statistics (all but the data)"""
        kw = dict(bscans=self.bscans, ascans=self.ascans, bins=bins)
        if self.fmt == F32:
            kw.update(depth=self.window, range=None if rng is None else (float(rng[0]), float(rng[1])))
        else:
            kw.update(samples=self.window, lo=None if rng is None else int(rng[0]), bin_width=None if rng is None else int(rng[1]))
        return kw

    def __repr__(self):
        return self.name


def poisoned(plan, fmt, region, poison=None):
    """the whole buffer of a handle with `region` ([nb][na][cnt] or [rows][cnt]) at the plan's place and poison everywhere else"""
    p = plan
    (fb, nb), (fa, na), (s0, cnt) = p.bscans, p.ascans, p.window
    if fmt == F32:
        buf = np.full((p.B, p.A, p.L), NAN, np.float32)
    else:
        buf = np.full((p.B, p.A, p.L), POISON[fmt] if poison is None else poison, np.int64)
    buf[fb:fb + nb, fa:fa + na, s0:s0 + cnt] = np.asarray(region).reshape(nb, na, cnt)
    return buf


def low_half(fmt, rng, shape):
    """random stored integers from the lower half of the container: below the poison, also after >> 4"""
    lo, hi = LIMITS[fmt]
    return rng.integers(lo, lo + (hi - lo) // 2, size=shape)


# ------------------------------------------------------------------------------------------------------------ 1. load forms
LOAD_HANDLE = (256, 12, 3)
LOAD_FORMATS = [F32] + list(sm.FORMATS)


def has_bitshift(fmt):
    return fmt != F32


def load_windows(fmt):
    """(s0, cnt, twin): the windows on multiples of V, and for each a twin one sample on (the scalar form)"""
    n = LOAD_HANDLE[0]
    L, V = (n // 2 if fmt == F32 else n), VECTOR[fmt]
    out = []
    for s0 in (0, V, 3 * V):
        for cnt in (1, V - 1, V, V + 1, 2 * V + 3, L - s0):
            out.append((s0, cnt, False))
            out.append((s0 + 1, min(cnt, L - s0 - 1), True))
    return out


def load_range(fmt, bitshift):
    """an explicit range with values on both sides of it: (bins, lo, hi) or (bins, lo, width)"""
    if fmt == F32:
        return 64, -0.5, 0.75
    lo, hi = (int(sm.decoded(np.int64(x), fmt[0], fmt[1], bitshift)) for x in LIMITS[fmt])
    span = hi - lo + 1  # (8 bit under bitshift: 16 values, 4 bins)
    width = max(1, span // 4 // 64)
    return min(64, span // 4 // width), lo + span // 8, width


def load_form_cases(fmt, bitshift=0):
    """one case per window; all of a format share one buffer (the same seed), cut differently"""
    n, a, b = LOAD_HANDLE
    bins, r0, r1 = load_range(fmt, bitshift)
    cases = []
    for s0, cnt, twin in load_windows(fmt):
        bsc, asc, win = (1, 2), (2, 9), (s0, cnt)

        def make(fmt=fmt, bsc=bsc, asc=asc, win=win):
            rng = np.random.default_rng(1000 + LOAD_FORMATS.index(fmt))
            plan = Plan(fmt, LOAD_HANDLE, bsc, asc, win)
            full = rng.standard_normal((b, a, plan.L)).astype(np.float32) if fmt == F32 else low_half(fmt, rng, (b, a, plan.L))
            return poisoned(plan, fmt, sm.region_of(full, bsc, asc, win))
        name = "%s-shift%d-s%d-c%d%s" % (FORMAT_ID[fmt], bitshift, s0, cnt, "-twin" if twin else "")
        runs = [(bins, (r0, r1))] + ([] if twin else [(16, None)])
        cases.append(Case(name, "scalar form" if twin else "vector form", LOAD_HANDLE, fmt, bsc, asc, win, make, runs, bitshift,
                          expect=dict(vector=not twin)))
    return cases


def load_offsets(fmt):
    """byte offsets of the misaligned device bases: 1, 2 and 3 elements (packed: bytes), for 8-bit data also 5 and 15 bytes"""
    if packed(fmt):
        return [1, 2, 3]
    eb = ELEM_BYTES[fmt]
    return [eb, 2 * eb, 3 * eb] + ([5, 15] if eb == 1 else [])


# ------------------------------------------------------------------------------------------------------------ 2. segment grid
GRID_HANDLES = {F32: (2048, 100, 22), (0, 8): (4096, 100, 22)}  # 9 011 200 bytes each; the last B-scan is never in a region
# (rows, bins): 2100 segments on 2048 workgroups; 1100 segments on the 1024 of more than 512 bins; 512 bins: every segment its own workgroup
GRID_CONFIGS = [(2100, 256), (1100, 513), (1100, 4096), (1100, 512)]


def _grid_buffer(fmt):
    n, a, b = GRID_HANDLES[fmt]
    rng = np.random.default_rng(77)
    L = n // 2 if fmt == F32 else n
    ramp = (np.linspace(0.0, 7.0, (b - 1) * a * L) % 1.0).reshape(b - 1, a, L)  # seven smooth sweeps: every region hits every bin
    if fmt == F32:
        v = (ramp * 12.0 - 1.0 + rng.standard_normal(ramp.shape) * 0.05).astype(np.float32)  # about [-1, 11]; the range is [0, 10]
        flat = v.reshape(-1)
        idx = rng.choice(flat.size, size=flat.size // 997, replace=False)
        flat[idx] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, size=idx.size)]
        buf = np.full((b, a, L), NAN, np.float32)
    else:
        v = np.clip(np.rint(ramp * 250.0 + rng.standard_normal(ramp.shape) * 3.0), 0, 254).astype(np.int64)
        buf = np.full((b, a, L), POISON[fmt], np.int64)
    buf[:b - 1] = v
    return buf


def grid_cases():
    cases = []
    for fmt, handle in GRID_HANDLES.items():
        n, a, b = handle
        L = n // 2 if fmt == F32 else n
        for rows, bins in GRID_CONFIGS:
            # 256 and more bins of an 8-bit container leave values on one side at most: [-40, 216) has the top ones and the poison above it
            explicit = (0.0, 10.0) if fmt == F32 else (-40, 1)
            cases.append(Case("%s-%drows-%dbins" % (FORMAT_ID[fmt], rows, bins), "more segments than workgroups" if bins != 512 else "a workgroup per segment",
                              handle, fmt, (0, rows // a), (0, a), (0, L), lambda fmt=fmt: _grid_buffer(fmt), [(bins, explicit), (bins, None)],
                              expect=dict(segments=rows, groups=min(rows, 1024 if bins > 512 else 2048), G=256, seg_rows=1)))
    return cases


# ------------------------------------------------------------------------------------------------------------ 3. staging slices
SLICE_F32_HANDLE = (8192, 2120, 2)  # the handle of tests/test_gpu_peak_crafted.py::test_host_source_beyond_one_staging_slice
SLICE_PACKED_HANDLE = (1001, 512, 100)


def _slice_f32_buffer():
    n, a, b = SLICE_F32_HANDLE
    vol = np.random.default_rng(21).standard_normal((b, a, n // 2), dtype=np.float32)
    vol[:, :4], vol[:, 4 + 2112:] = NAN, NAN
    return vol


def _slice_packed_buffer():
    n, a, b = SLICE_PACKED_HANDLE
    return np.random.default_rng(22).integers(0, 256, size=n * a * b * 3 // 2, dtype=np.uint8)  # any byte string is valid packed data


def slice_cases():
    """the host source of each is staged in two slices whose border lies inside a B-scan; all cases of a handle share one buffer"""
    cases = [Case("f32-2-slices", "staging slices", SLICE_F32_HANDLE, F32, (0, 2), (4, 2112), (12, 61), _slice_f32_buffer,
                  [(256, (-2.0, 2.0)), (256, None)], expect=dict(seg_rows=16, slice_segments=255, borders=[4080]))]
    for fmt in ((1, 12), (2, 12)):
        lo = 100 if fmt[0] == 1 else -1900
        cases.append(Case("%s-2-slices" % FORMAT_ID[fmt], "staging slices, parity", SLICE_PACKED_HANDLE, fmt, (0, 100), (0, 512), (7, 61),
                          _slice_packed_buffer, [(256, (lo, 15)), (64, None)], as_bytes=True,
                          expect=dict(seg_rows=32, slice_segments=1390, borders=[44480], border_in_bscan=448)))
        cases.append(Case("%s-2-slices-part-bscans" % FORMAT_ID[fmt], "staging slices, parity, one copy per B-scan", SLICE_PACKED_HANDLE, fmt,
                          (0, 100), (3, 500), (9, 64), _slice_packed_buffer, [(256, (lo, 15))], as_bytes=True,
                          expect=dict(seg_rows=32, slice_segments=1390, borders=[44480], border_in_bscan=480)))
    return cases


# ------------------------------------------------------------------------------------------------------------ 4. wave-uniform add
WAVE_HANDLE = (1024, 32, 4)
WAVE_BINS = (1, 2, 8, 4096)
U16 = (0, 12)


def wave_ranges(fmt):
    """the explicit range of each bin count: eight levels, level i in bin i of 8 (and all in one of 1, in distinct ones of 4096)"""
    if fmt == F32:
        return [(bins, (0.0, 8.0)) for bins in WAVE_BINS]
    return [(1, (50, 1600)), (2, (50, 800)), (8, (50, 200)), (4096, (50, 1))]


def _wave_values(fmt, plan):
    """runs of one level over many whole wave instructions, their borders anywhere; runs of excluded values; exceptions at lane 0, 63
    and 17 of every seventh wave instruction that would otherwise be uniform with every lane active"""
    if fmt == F32:
        level = lambda i: np.float32(i + 0.5)
        out_run, exceptions = NAN, [NAN, np.float32(-1.0), np.float32(9.0), "next", "prev"]
        vals = np.empty(plan.rows * plan.window[1], np.float32)
    else:
        level = lambda i: 150 + 200 * i
        out_run, exceptions = 7, [7, 60000, "next", "prev"]
        vals = np.empty(plan.rows * plan.window[1], np.int64)
    rng = np.random.default_rng(404)
    lv = np.empty(vals.size, np.int64)  # the level of each value, -1 in an excluded run
    pos = i = 0
    while pos < vals.size:
        ln = int(rng.integers(3, 9)) * 64 * plan.V + int(rng.integers(1, 64 * plan.V))
        lv[pos:pos + ln] = -1 if i % 5 == 3 else int(rng.integers(0, 8))
        pos, i = pos + ln, i + 1
    for k in range(-1, 8):
        vals[lv == k] = out_run if k < 0 else level(k)
    n = 0
    for m in plan.lane_map():
        for q in range(m.shape[0]):
            for j in range(m.shape[1]):
                idx = m[q, j]
                if idx.min() < 0 or lv[idx[0]] < 0 or np.any(lv[idx] != lv[idx[0]]):
                    continue
                n += 1
                if n % 7:
                    continue
                lane = (0, 63, 17)[(n // 7) % 3]
                e = exceptions[(n // 21) % len(exceptions)]
                k = int(lv[idx[0]])
                if isinstance(e, str):
                    e = level(k + 1 if (e == "next" and k < 7) or k == 0 else k - 1)
                vals[idx[lane]] = e
    return vals


def wave_cases():
    cases = []
    for fmt, win in ((F32, (4, 203)), (U16, (8, 517))):
        bsc, asc = (0, 4), (1, 30)

        def make(fmt=fmt, win=win, bsc=bsc, asc=asc):
            plan = Plan(fmt, WAVE_HANDLE, bsc, asc, win)
            return poisoned(plan, fmt, _wave_values(fmt, plan))
        cases.append(Case("%s-waves" % FORMAT_ID[fmt], "wave-uniform add", WAVE_HANDLE, fmt, bsc, asc, win, make, wave_ranges(fmt)))
    return cases


# ------------------------------------------------------------------------------------------------------------ 5. binning edges
EDGE_HANDLE = (1024, 32, 4)
CORRECTED_WIDTHS = (49, 103, 107)  # the float64 reciprocal quotient of some multiple is one too small (the q++ of stats_bin_raw)
CONTROL_WIDTH = 1000003
EDGE_LOS = {(0, 32): (0, -5, -2 ** 40), (5, 32): (0, -1000, -2 ** 31, -2 ** 40), (4, 16): (0, -3000, -2 ** 40)}


def uncorrected_bin(d, width):
    """stats_bin_raw without its correction: the float64 product with the reciprocal, truncated"""
    return int(float(d) * (1.0 / float(width)))


def _edge_ints(fmt, lo, width, bins):
    """lo + m * width + {-1, 0, 1} for every m up to bins that the container holds, the last value below the limit and the first at it;
    where the container holds none of them (lo = -2**40), its own extremes and random values"""
    fl, fh = LIMITS[fmt]
    m = np.arange(bins + 1, dtype=object)
    v = np.concatenate([lo + m * width - 1, lo + m * width, lo + m * width + 1, np.array([lo + bins * width - 1, lo + bins * width], dtype=object)])
    v = np.array([x for x in v if fl <= x <= fh], dtype=np.int64)
    if v.size < 16:
        v = np.concatenate([v, [fl, fh], np.random.default_rng(5).integers(fl, fh, size=64, endpoint=True)])
    n, a, b = EDGE_HANDLE
    return np.resize(v, (b, a, n))


def raw_edge_cases():
    cases = []
    n, a, b = EDGE_HANDLE
    for fmt, los in EDGE_LOS.items():
        for lo in los:
            for width in CORRECTED_WIDTHS + (CONTROL_WIDTH,):
                bins = 4096
                cases.append(Case("%s-lo%d-w%d" % (FORMAT_ID[fmt], lo, width), "stats_bin_raw", EDGE_HANDLE, fmt, (0, b), (0, a), (0, n),
                                  lambda fmt=fmt, lo=lo, width=width, bins=bins: _edge_ints(fmt, lo, width, bins), [(bins, (lo, width))],
                                  expect=dict(corrected=width in CORRECTED_WIDTHS and lo > -2 ** 40)))
    for fmt in ((0, 32), (5, 32)):
        def make(fmt=fmt):
            fl, fh = LIMITS[fmt]
            v = np.random.default_rng(6).integers(fl, fh, size=(b, a, n), endpoint=True)
            v.reshape(-1)[:4] = [fl, fh, fl + 1, fh - 1]
            return v
        cases.append(Case("%s-whole-range-auto" % FORMAT_ID[fmt], "derived width up to 2**32", EDGE_HANDLE, fmt, (0, b), (0, a), (0, n), make,
                          [(1, None), (3, None), (4096, None)]))
    return cases


def _f32(x):
    return np.float32(x)


def processed_edge_cases():
    n, a, b = EDGE_HANDLE
    L = n // 2
    tiny = np.float32(1e-45)  # the smallest subnormal
    one_up = np.nextafter(_f32(1), _f32(2))
    sub = _f32(1e-40)
    sub_up = np.nextafter(sub, _f32(1))

    def tiled(v):
        return lambda: np.resize(np.asarray(v, np.float32), (b, a, L))

    def around(*xs):
        out = []
        for x in xs:
            x = _f32(x)
            out += [x, np.nextafter(x, _f32(-np.inf)), np.nextafter(x, _f32(np.inf))]
        return out
    subnormals = [tiny * _f32(k) for k in range(-5, 6)] + [-0.0, 1e-38, -1e-38, 1.1754944e-38]
    cases = []
    for name, lo, hi in (("one-ulp-at-1", _f32(1), one_up), ("zero-to-tiny", _f32(0), tiny), ("minus-tiny-to-zero", -tiny, _f32(0)),
                         ("one-ulp-subnormal", sub, sub_up)):
        clamps = float(8) / (float(hi) - float(lo)) > sm.FLT_MAX
        cases.append(Case("f32-" + name, "scale clamps to FLT_MAX" if clamps else "one ulp wide", EDGE_HANDLE, F32, (0, b), (0, a), (0, L),
                          tiled(around(lo, hi) + subnormals + around(1.0)), [(bins, (lo, hi)) for bins in (1, 8, 4096)], expect=dict(clamps=clamps)))
    rng = np.random.default_rng(8)
    wide = (rng.uniform(-1.0, 1.0, size=4096) * 3.4e38).astype(np.float32)
    cases.append(Case("f32-wide", "v - lo overflows to inf", EDGE_HANDLE, F32, (0, b), (0, a), (0, L),
                      tiled(np.concatenate([wide, around(-3e38, 3e38, 0.0, 4.02e37, 4.03e37)])), [(bins, (-3e38, 3e38)) for bins in (1, 8, 4096)],
                      expect=dict(overflows=True)))
    for name, x in (("adjacent-at-1", _f32(1)), ("adjacent-subnormal", tiny * _f32(3)), ("adjacent-at-max", np.nextafter(_f32(np.inf), _f32(0)))):
        y = np.nextafter(x, _f32(-np.inf))
        cases.append(Case("f32-" + name, "autoRange on two adjacent floats", EDGE_HANDLE, F32, (0, b), (0, a), (0, L), tiled([y, x, x]),
                          [(bins, None) for bins in (1, 2, 4096)]))
    return cases


# ------------------------------------------------------------------------------------------------------------ 6. moments
MOMENT_HANDLES = ((1024, 32, 4), (1024, 48, 4))
MOMENT_SUB = ((1, 2), (3, 20))  # bscans, ascans of the sub-region; its window is (8, 200) of float32, (8, 400) of raw samples


def _moment_values(kind, rng, size):
    if kind == "2^23+U64":
        return (2.0 ** 23 + rng.integers(0, 64, size=size)).astype(np.float32)
    if kind == "1e30-ulps":
        return (np.float32(1e30).astype(np.float64) * (1.0 + rng.integers(0, 64, size=size) * 2.0 ** -23)).astype(np.float32)
    if kind == "-1e-30-ulps":
        return (np.float32(-1e-30).astype(np.float64) * (1.0 + rng.integers(0, 64, size=size) * 2.0 ** -23)).astype(np.float32)
    if kind == "outlier-3e38":
        v = np.ones(size, np.float32)
        v[size // 3] = 3e38
        return v
    if kind == "all-but-one":
        v = np.full(size, 3.25, np.float32)
        v[2 * size // 3] = 3.5
        return v
    if kind == "u32-top":
        return 2 ** 32 - 1 - rng.integers(0, 9, size=size)
    if kind == "i32-bottom":
        return -2 ** 31 + rng.integers(0, 9, size=size)
    assert kind == "i16-constant"
    return np.full(size, -12345, np.int64)


MOMENT_KINDS = [("2^23+U64", F32), ("1e30-ulps", F32), ("-1e-30-ulps", F32), ("outlier-3e38", F32), ("all-but-one", F32),
                ("u32-top", (0, 32)), ("i32-bottom", (5, 32)), ("i16-constant", (4, 16))]


def moment_cases():
    """each kind as the whole region of the first handle and as the same sub-region of both handles (the same values: the header says the
    bits depend on the region's shape only)"""
    cases = []
    for kind, fmt in MOMENT_KINDS:
        for handle, sub in ((MOMENT_HANDLES[0], False), (MOMENT_HANDLES[0], True), (MOMENT_HANDLES[1], True)):
            n, a, b = handle
            L = n // 2 if fmt == F32 else n
            bsc, asc, win = (MOMENT_SUB + ((8, 200 if fmt == F32 else 400),)) if sub else ((0, b), (0, a), (0, L))

            def make(kind=kind, fmt=fmt, handle=handle, bsc=bsc, asc=asc, win=win):
                plan = Plan(fmt, handle, bsc, asc, win)
                v = _moment_values(kind, np.random.default_rng(600), plan.rows * win[1])
                # (u32-top: the values are at the top of the container, the poison is its lowest value)
                return poisoned(plan, fmt, v, poison=0 if kind == "u32-top" else None)
            cases.append(Case("%s-%s-A%d" % (kind, "sub" if sub else "whole", a), "moments", handle, fmt, bsc, asc, win, make, [(64, None)],
                              expect=dict(kind=kind, sub=sub)))
    return cases


def exact_moments(values):
    """(mean, population stddev) of float32 or integer values from exact rational arithmetic, rounded once at the end"""
    import math
    from fractions import Fraction
    v = np.asarray(values).ravel()
    if v.dtype.kind == "f":
        ints = [p * (2 ** 149 // q) for p, q in (float(x).as_integer_ratio() for x in v)]  # every finite float32 is a multiple of 2**-149
        unit = Fraction(1, 2 ** 149)
    else:
        ints, unit = [int(x) for x in v], Fraction(1)
    n, s, q = len(ints), sum(ints), sum(x * x for x in ints)
    mean = Fraction(s, n) * unit
    var = Fraction(n * q - s * s, n * n) * unit * unit
    # sqrt of a correctly rounded float64: one more rounding, far below the 1e-12 this is used at; scaled to stay in range
    if var == 0:
        return float(mean), 0.0
    e = (var.numerator.bit_length() - var.denominator.bit_length()) // 2 * 2
    return float(mean), math.sqrt(float(var / Fraction(2) ** e)) * 2.0 ** (e // 2)
