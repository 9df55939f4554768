"""Crafted inputs for the phase extraction (include/octpipe.h "phase extraction"): one accumulate case per instance and launch shape of
oct_phase_accumulate_kernel<F, VEC> (csrc/phase_extract.h, csrc/pipe_phase.hip launchAccumulate), and averaged interferograms whose
phase is NOT monotone, so that the lane scans and both clamps of oct_phase_extract_kernel have work to do.
tests/test_phase_cases.py proves on the model alone (tests/phase_model.py) that every case reaches what it declares;
tests/test_gpu_phase_crafted.py runs exactly these cases on the device.  Seeded generators only: no device, no files.

An accumulate case is (format, bitDepth, N, A, B, bitshift, source, base offset, calls, values): `source` is "host", "device" (a
16-byte aligned tensor) or "sliced" (a device tensor whose data starts `offset` bytes into a 16-byte aligned allocation); a call is
(firstAscan, ascanCount) or (firstAscan, ascanCount, source) where one accumulator is fed from two memories."""
import numpy as np

import phase_model as pm

THREADS, UNROLL = 256, 4  # PHASE_THREADS, PHASE_UNROLL of csrc/phase_extract.h
LENGTHS = [256, 512, 1024, 2048, 4096]
FORMATS = [(0, 8), (0, 12), (0, 32), (1, 12), (2, 12), (3, 8), (4, 16), (5, 32)]
FORMAT_ID = {(0, 8): "u8", (0, 12): "u16", (0, 16): "u16", (0, 32): "u32", (1, 12): "p12u", (2, 12): "p12s", (3, 8): "i8", (4, 16): "i16", (5, 32): "i32"}


# ---------------------------------------------------------------------------------------------------------------------- values
def _encode(ints, fmt, bit_depth):
    """raw bytes of integer samples [lines, n] in sample format fmt (OCTPIPE_FORMAT_*) and their decoded integer (before bitshift).
    Packed 12 bit: the samples of the whole buffer pair up in order (two per byte triple), so a row of odd length starts inside a
    triple on every odd row; the bytes come back flat then, [lines, 1.5 n] otherwise."""
    if fmt in (1, 2):
        u = (ints & 0xFFF).astype(np.uint32)
        flat = u.reshape(-1)
        s0, s1 = flat[0::2], flat[1::2]
        b = np.stack([s0 & 0xFF, ((s0 >> 8) & 0xF) | ((s1 & 0xF) << 4), s1 >> 4], axis=-1).astype(np.uint8)
        dec = u.astype(np.int64) if fmt == 1 else ((u.astype(np.int64) ^ 0x800) - 0x800)
        return (b.reshape(ints.shape[0], -1) if ints.shape[-1] % 2 == 0 else b.reshape(-1)), dec
    dt = {3: np.int8, 4: np.int16, 5: np.int32}.get(fmt) or (np.uint8 if bit_depth <= 8 else np.uint16 if bit_depth <= 16 else np.uint32)
    arr = ints.astype(dt)
    return arr, arr.astype(np.int64)


def value_range(fmt, bit_depth):
    """[lo, hi] of the stored integer"""
    if fmt == 1:
        return 0, 4095
    if fmt == 2:
        return -2048, 2047
    if fmt in (3, 4, 5):
        bits = {3: 8, 4: 16, 5: 32}[fmt]
        return -2 ** (bits - 1), 2 ** (bits - 1) - 1
    return 0, 2 ** min(bit_depth, 32) - 1


def _random_ints(rng, shape, fmt, bit_depth):
    if fmt in (1, 2):
        return rng.integers(0, 4096, size=shape)
    if fmt == 3:
        return rng.integers(-128, 128, size=shape)
    if fmt == 4:
        return rng.integers(-32768, 32768, size=shape)
    if fmt == 5:
        return rng.integers(-2 ** 31, 2 ** 31, size=shape)
    return rng.integers(0, 2 ** min(bit_depth, 32), size=shape, dtype=np.uint64).astype(np.int64)


def _extreme_ints(rng, shape, fmt, bit_depth):
    """the format's smallest and largest value only, drawn per sample (both land on both halves of a packed pair)"""
    lo, hi = value_range(fmt, bit_depth)
    return np.where(rng.integers(0, 2, size=shape) == 1, np.int64(hi), np.int64(lo))


def _row_ints(shape, fmt, bit_depth):
    """row r holds the constant r + 1 (modulo the format's largest value): a row counted twice or skipped changes every sum"""
    hi = value_range(fmt, bit_depth)[1]
    return np.broadcast_to(((np.arange(shape[0], dtype=np.int64) % hi) + 1)[:, None], shape).copy()


# ---------------------------------------------------------------------------------------------------------------------- launch rule
def elem_bytes(fmt, bit_depth):
    """bytes per sample (packed 12 bit: 0, 1.5 in truth)"""
    if fmt in (1, 2):
        return 0
    return {3: 1, 4: 2, 5: 4}.get(fmt) or (1 if bit_depth <= 8 else 2 if bit_depth <= 16 else 4)


def vector_samples(fmt, bit_depth):
    return 8 if fmt in (1, 2) else 16 // elem_bytes(fmt, bit_depth)


def accumulate_form(fmt, bit_depth, n, base_offset_bytes, host):
    """(vec, chunks, rowsPerPass, colBlocks) as launchAccumulate (csrc/pipe_phase.hip) chooses them.  A host source is staged, so its
    base is aligned."""
    base = 0 if host else int(base_offset_bytes)
    if fmt in (1, 2):
        vec = n % 8 == 0 and base % 4 == 0
    else:
        vec = (n * elem_bytes(fmt, bit_depth)) % 16 == 0 and base % 16 == 0
    chunks = n // vector_samples(fmt, bit_depth) if vec else n
    rows_per_pass = THREADS // chunks if chunks <= THREADS else 1
    col_blocks = 1 if rows_per_pass > 1 else (chunks + THREADS - 1) // THREADS
    return vec, chunks, rows_per_pass, col_blocks


def row_groups(rows, rows_per_pass, col_blocks, cus=256):
    """rowGroups of one launch over `rows` rows"""
    passes = (rows + rows_per_pass - 1) // rows_per_pass
    return min(max(1, cus * 8 // col_blocks), max(1, passes // UNROLL))


def lane_row_counts(rows, rows_per_pass, groups):
    """how many rows each (row group, row offset) of a launch sums: the unrolled loop takes them four at a time, the rest is its tail"""
    stride = groups * rows_per_pass
    return [len(range(r0, rows, stride)) for r0 in range(stride)]


def stage_plan(fmt, n, first, count):
    """(lead, rows) of a host call: the rows the kernel is given of the staged copy start `lead` rows into it (csrc/phase_stage.h; a
    call this small is one slice)"""
    lead = (first & 1) if (fmt in (1, 2) and n % 2 == 1) else 0
    return lead, count


# ---------------------------------------------------------------------------------------------------------------------- accumulate
OFFSET = {0: 0, 1: 1, 2: 2, 4: 4}


def misaligned_offset(fmt, bit_depth):
    """bytes into a 16-byte aligned allocation at which a sliced source starts: 2 for 16-bit, 1 for 8-bit, 4 for 32-bit, 3 for packed"""
    e = elem_bytes(fmt, bit_depth)
    return 3 if e == 0 else {1: 1, 2: 2, 4: 4}[e]


class AccCase:
    def __init__(self, name, fmt, bit_depth, n, a, b, bitshift, source, calls, values="random", seed=0):
        self.name, self.fmt, self.bit_depth, self.n, self.a, self.b, self.bitshift = name, fmt, bit_depth, n, a, b, bitshift
        self.source = source
        self.offset = misaligned_offset(fmt, bit_depth) if source == "sliced" else 0
        self.calls = [(c[0], c[1], c[2] if len(c) > 2 else source) for c in calls]
        self.values, self.seed = values, seed
        assert a * b <= 600 and all(f + c <= a * b and c >= 1 for f, c, _ in self.calls), name
        assert fmt not in (1, 2) or (n * a * b) % 2 == 0, name

    def __repr__(self):
        return self.name

    @property
    def lines(self):
        return self.a * self.b

    def offset_of(self, source):
        return misaligned_offset(self.fmt, self.bit_depth) if source == "sliced" else 0

    def form(self, source=None):
        source = self.source if source is None else source
        return accumulate_form(self.fmt, self.bit_depth, self.n, self.offset_of(source), source == "host")

    def launches(self):
        """(vec, rowsPerPass, colBlocks, rowGroups, firstRow, rows) of every kernel launch of the case"""
        out = []
        for first, count, source in self.calls:
            vec, _, rpp, cb = self.form(source)
            lead = stage_plan(self.fmt, self.n, first, count)[0] if source == "host" else first
            out.append((vec, rpp, cb, row_groups(count, rpp, cb), lead, count))
        return out

    def data(self):
        """(raw array as the handle takes it, decoded integers [lines, n])"""
        shape = (self.lines, self.n)
        rng = np.random.default_rng(self.seed)
        if self.values == "random":
            ints = _random_ints(rng, shape, self.fmt, self.bit_depth)
        elif self.values == "extremes":
            ints = _extreme_ints(rng, shape, self.fmt, self.bit_depth)
        else:
            ints = _row_ints(shape, self.fmt, self.bit_depth)
        return _encode(ints, self.fmt, self.bit_depth)

    def expected(self, dec, calls=None):
        """(mean float32 [n], count) of the calls: float32((int64 sum / count) * scale) as octpipe_phase_mean defines it"""
        u32 = self.fmt == 0 and self.bit_depth > 16
        val = dec if (not self.bitshift or u32) else (dec >> 4)
        scale = 2.0 ** -32 if (u32 and self.bitshift) else 1.0
        total, count = np.zeros(self.n, np.int64), 0
        for first, cnt, _ in (self.calls if calls is None else calls):
            total += val[first:first + cnt].sum(axis=0)
            count += cnt
        return ((total / count) * scale).astype(np.float32), count

    def twin_calls(self):
        """the same rows for a second handle: neighbouring calls joined into one, from the other memory and another alignment"""
        other = {"host": "sliced", "device": "host", "sliced": "host"}
        joined = []
        for first, count, source in self.calls:
            if joined and joined[-1][0] + joined[-1][1] == first and joined[-1][2] == source:
                joined[-1] = (joined[-1][0], joined[-1][1] + count, source)
            else:
                joined.append((first, count, source))
        return [(f, c, other[s]) for f, c, s in joined]


def _split(lines):
    """calls of 1, 2, 3 and 5 A-scans and the rest, side by side over the whole buffer (odd firstAscan: 1, 3), then the whole buffer"""
    return [(0, 1), (1, 2), (3, 3), (6, 5), (11, lines - 11), (0, lines)]


def _accumulate_cases():
    cases = []
    # 1. every (format, form) pair at N = 1024, 16 x 4 A-scans: the aligned tensor and the staged host copy take the vector form
    #    (rowsPerPass 4 / 2 / 1), the sliced tensor the scalar form in four column blocks; bitshift alternates
    for i, (fmt, bd) in enumerate(FORMATS):
        fid = FORMAT_ID[(fmt, bd)]
        cases.append(AccCase("vector-%s-1024" % fid, fmt, bd, 1024, 16, 4, i & 1, "device" if i & 2 else "host", _split(64), seed=100 + i))
        cases.append(AccCase("scalar-%s-1024" % fid, fmt, bd, 1024, 16, 4, 1 - (i & 1), "sliced", _split(64) + [(37, 3), (5, 7), (2, 11), (5, 37), (5, 38), (5, 39)], seed=200 + i))
    # 2. the format's extremes, through the scalar form (one sample per load: both halves of a packed pair, every sign extension)
    #    with the vector form as the twin's; both bitshifts for the signed 12-bit and 8-bit containers, whose >> 4 is arithmetic
    for i, (fmt, bd) in enumerate(FORMATS + [(0, 16)]):
        fid = FORMAT_ID[(fmt, bd)] + ("-16" if bd == 16 and fmt == 0 else "")
        for shift in ((0, 1) if fmt in (2, 3, 4, 5) else (i & 1,)):
            cases.append(AccCase("extremes-%s-shift%d" % (fid, shift), fmt, bd, 256, 8, 3, shift, "sliced", [(1, 5), (0, 24), (23, 1)], "extremes", seed=300 + i))
    # 3. the vector form with colBlocks > 1 and rowGroups > 1: 150 rows; 37 = 4 * 9 + 1 rows over 9 row groups (one lane goes round
    #    the unrolled loop once and takes a fifth row in the tail), 38 and 39 likewise; 11 rows over 2 groups leave tails of 2 and 1, 7
    #    rows in one group a tail of 3 (rowGroups = passes / 4, so a lane never has 7 rows when there are two groups)
    for fmt, bd, n in ((0, 12, 4096), (0, 32, 2048), (5, 32, 2048)):
        cases.append(AccCase("vector-%s-%d-colblocks" % (FORMAT_ID[(fmt, bd)], n), fmt, bd, n, 30, 5, 0, "device", [(5, 37), (0, 150), (1, 38), (111, 39), (3, 7), (2, 11)], seed=400 + n + fmt))
    # 4. the vector form with rowsPerPass = 16 (uint8, N = 256): counts below rowsPerPass, a firstAscan that is odd and no multiple
    #    of it, and 16 * 9 * 4 + 16 + 5 = 597 rows for a tail
    cases.append(AccCase("vector-u8-256-rpp16", 0, 8, 256, 100, 6, 0, "device", [(3, 597), (7, 5), (9, 1), (0, 600, "host"), (21, 15)], seed=500))
    cases.append(AccCase("vector-i8-1024-rpp4", 3, 8, 1024, 50, 4, 1, "host", [(1, 3), (5, 2), (0, 200), (9, 37, "device"), (13, 150)], seed=501))
    cases.append(AccCase("vector-i16-1024-rpp2", 4, 16, 1024, 50, 4, 0, "device", [(1, 1), (3, 75), (0, 200, "host"), (7, 38)], seed=502))
    # 5. the scalar form at the lengths that are no power of two: N = 1000 in four column blocks with a partial last one, N = 130 as
    #    one partial block (260 bytes per row), N = 96 with rowsPerPass = 2 and 64 idle threads; N = 96 in uint8 is 6 vector loads per
    #    row: rowsPerPass = 42 and 4 idle threads
    cases.append(AccCase("scalar-u16-1000", 0, 12, 1000, 16, 4, 0, "sliced", _split(64) + [(5, 37)], seed=600))
    cases.append(AccCase("scalar-u16-130", 0, 12, 130, 16, 2, 0, "host", [(3, 20), (0, 32, "device"), (1, 1)], seed=601))
    cases.append(AccCase("scalar-u16-96-rpp2", 0, 12, 96, 20, 5, 1, "sliced", [(0, 1), (1, 2), (3, 3), (6, 5), (11, 89), (0, 100), (5, 37), (9, 38)], seed=602))
    cases.append(AccCase("scalar-i8-96-rpp2", 3, 8, 96, 20, 5, 1, "sliced", [(1, 1), (3, 39), (0, 100)], "extremes", seed=603))
    cases.append(AccCase("vector-u8-96-rpp42", 0, 8, 96, 100, 6, 0, "host", [(1, 5), (7, 41), (0, 600), (45, 43), (3, 389)], seed=604))
    # 6. row r holds r + 1: every row of every split counted once
    cases.append(AccCase("rows-u16-512", 0, 12, 512, 100, 6, 0, "device", [(0, 1), (1, 2), (3, 3), (6, 5), (11, 37), (48, 552), (0, 600, "host"), (299, 2, "sliced")], "rows"))
    cases.append(AccCase("rows-p12s-1024", 2, 12, 1024, 100, 6, 0, "sliced", [(0, 7), (7, 593), (1, 37, "host"), (0, 600, "device"), (598, 2, "device")], "rows"))
    return cases


ACCUMULATE_CASES = _accumulate_cases()

# packed 12 bit on rows of odd length: (format, N, A, B); firstAscan 0, 1, 2, 3 and the whole buffer, host and device
PACKED_ODD = [(fmt, n, a, b) for fmt in (1, 2) for n, a, b in ((129, 4, 2), (255, 2, 3))]
PACKED_ODD_FIRST = [0, 1, 2, 3]


def packed_odd_case(fmt, n, a, b, source, bitshift=0):
    lines = a * b
    calls = [(f, min(2, lines - f)) for f in PACKED_ODD_FIRST] + [(f, lines - f) for f in PACKED_ODD_FIRST[1:]] + [(0, lines)]
    return AccCase("packed-odd-%s-%d-%s" % (FORMAT_ID[(fmt, 12)], n, source), fmt, 12, n, a, b, bitshift, source, calls, "random", seed=700 + n + fmt)


def stale_host_rows(raw_flat, n, first, count):
    """the bytes the host path copied BEFORE csrc/phase_stage.h, for a packed buffer of `lines` rows: offset first * floor(1.5 n),
    count * floor(1.5 n) bytes (the arithmetic of the defect, kept for the record and for test_phase_cases.py)"""
    row_bytes = (3 * n) // 2
    return raw_flat[first * row_bytes:first * row_bytes + count * row_bytes]


def decode_packed(staged, idx, signed):
    """sample idx of a packed byte array as decode_sample (csrc/sample_decode.h) reads it"""
    t = (idx >> 1) * 3
    v = (int(staged[t + 1]) >> 4) | (int(staged[t + 2]) << 4) if idx & 1 else int(staged[t]) | ((int(staged[t + 1]) & 15) << 8)
    return ((v ^ 0x800) - 0x800) if signed else v


# ---------------------------------------------------------------------------------------------------------------------- extract
def two_tone_mean(n, k1, k2, r, amp=600, phase=0.7, offset=2048):
    """offset + amp cos(2 pi k1 j / n) + r amp cos(2 pi k2 j / n + phase) in float32.  A positive-band signal loses monotone phase only
    near the nulls of its envelope; two tones of nearly equal height at low bins make each dip many samples wide, and the phase runs
    backwards across it."""
    j = np.arange(n, dtype=np.float64)
    return (offset + amp * np.cos(2.0 * np.pi * k1 * j / n) + r * amp * np.cos(2.0 * np.pi * k2 * j / n + phase)).astype(np.float32)


class ExtractCase:
    def __init__(self, name, n, mean, peak, a, b, window_raw=False, hann_peak=False):
        self.name, self.n, self._mean, self.peak, self.a, self.b = name, n, mean, peak, a, b
        self.window_raw, self.hann_peak = window_raw, hann_peak
        self._model = {}

    def __repr__(self):
        return self.name

    def mean(self):
        return self._mean()

    def kwargs(self):
        """the arguments of Pipeline.extract_resample_curve behind mean="""
        return dict(peak=self.peak, window_raw=self.window_raw, hann_peak=self.hann_peak, ignore_first=self.a, ignore_last=self.n - 1 - self.b)

    def model(self, transform_dtype=np.float64):
        """tests/phase_model.py extract of the case, computed once per precision and shared (do not write into it)"""
        key = np.dtype(transform_dtype).name
        if key not in self._model:
            self._model[key] = pm.extract(self.mean(), self.peak[0], self.peak[1], self.window_raw, self.hann_peak, self.a, self.n - 1 - self.b,
                                          transform_dtype=transform_dtype)
        return self._model[key]


def changed_runs(w, n):
    """[(first, last, lane segments touched)] of the runs where the monotone envelope changed psi (segments of P = n / 64 samples)"""
    p = n // 64
    ch = np.nonzero(w["psi_mono"] != w["psi"])[0]
    runs = []
    for c in ch:
        if runs and runs[-1][1] == c - 1:
            runs[-1][1] = c
        else:
            runs.append([c, c])
    return [(int(s), int(e), int(e // p - s // p + 1)) for s, e in runs]


def domain(mono, n):
    """the j whose curve entry is an interpolated one: mono[0] <= j < mono[-1]"""
    j = np.arange(n, dtype=np.float64)
    return (j >= mono[0]) & (j < mono[-1])


def near_clamp(mono, n, atol):
    """the j within atol of either end of the domain: rounding may put them on either side of a clamp"""
    j = np.arange(n, dtype=np.float64)
    return (np.abs(j - mono[0]) <= atol) | (np.abs(j - mono[-1]) <= atol)


def calibration_mean(n, seed):
    return pm.calibration_raw(n, 64, seed=seed).astype(np.float64).mean(axis=0).astype(np.float32)


def _extract_cases():
    cases = []
    for n in LENGTHS:
        def tt(k1, k2, r, n=n):
            return lambda: two_tone_mean(n, k1, k2, r)
        cases.append(ExtractCase("tones-3-8-%d" % n, n, tt(3, 8, 0.95), (2, 12), n // 2 + 3, n - 5))
        cases.append(ExtractCase("tones-4-7-%d" % n, n, tt(4, 7, 0.97), (2, 12), n // 2 + 3, n - 5))
        # the anchor at sample 0 (the n == 0 skip of the jump scan, lane 0's runLo, ignoreLast = 0) and inside the last lane (the
        # minimum scan crosses all 64 lanes)
        cases.append(ExtractCase("tones-3-8-%d-anchor-0" % n, n, tt(3, 8, 0.95), (2, 12), 0, n - 1))
        cases.append(ExtractCase("tones-3-8-%d-anchor-last-lane" % n, n, tt(3, 8, 0.95), (2, 12), n - 12, n - 2))
        # both windows: tones at equal weights of the band's Hann window (bins 4 and 10 of [2, 12])
        cases.append(ExtractCase("tones-4-10-%d-windows" % n, n, tt(4, 10, 0.95), (2, 12), n // 2 + 3, n - 5, window_raw=True, hann_peak=True))
        # the clean fringe with a short [a, b]: psi(N-1) stays below N-1, so the last entries take the `y >= last` clamp
        cases.append(ExtractCase("fringe-%d-short-b" % n, n, (lambda n=n: calibration_mean(n, n + 1)), (int(0.2 * n), int(0.4 * n)), n // 16, n - 1 - n // 4,
                                 hann_peak=True))
    return cases


EXTRACT_CASES = _extract_cases()


def silent_band_case(n):
    """a two-tone mean whose band [20, 40] holds neither tone: no calibration signal.  The tones sit at N/4 and N/2, so the float32
    samples have period 4 and every other bin is exactly zero in any order of the transform's sums -- tones elsewhere would leave
    rounding noise in the band, and noise has a phase."""
    return ExtractCase("tones-%d-silent-band" % n, n, lambda: two_tone_mean(n, n // 4, n // 2, 0.95), (20, 40), n // 2 + 3, n - 5)
