"""numpy restatement of the image statistics definition (include/octpipe.h "image statistics"), the yardstick of
tests/test_image_statistics.py and tests/test_gpu_image_statistics.py."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def region_of(buf, bscans, ascans, samples):
    """the region's elements of one buffer [B][A][L] in (b, a, s) order"""
    (fb, nb), (fa, na), (fs, ns) = bscans, ascans, samples
    return buf[fb:fb + nb, fa:fa + na, fs:fs + ns]


def processed_scale(bins, lo, hi):
    if lo == hi:
        return np.float32(0.0)
    return np.float32(min(float(bins) / (float(hi) - float(lo)), FLT_MAX))


def processed(values, bins, lo=None, hi=None):
    """statistics of float32 values; lo = hi = None: autoRange"""
    v = np.asarray(values, dtype=np.float32).ravel()
    fin = np.isfinite(v)
    f = v[fin]
    if lo is None:
        lo, hi = (np.float32(f.min()), np.float32(f.max())) if f.size else (np.float32(np.nan), np.float32(np.nan))
    lo, hi = np.float32(lo), np.float32(hi)
    hist = np.zeros(bins, np.uint64)
    under = over = 0
    if f.size and np.isfinite(lo):
        scale = processed_scale(bins, lo, hi)
        under = int(np.count_nonzero(f < lo))
        over = int(np.count_nonzero(f > hi))
        inr = f[(f >= lo) & (f <= hi)]
        with np.errstate(over="ignore", invalid="ignore"):
            t = (inr - lo).astype(np.float32) * scale  # two float32 roundings
        fl = np.floor(t)
        b = np.where(fl >= bins - 1, bins - 1, fl).astype(np.int64)
        hist = np.bincount(b, minlength=bins).astype(np.uint64)
    d = f.astype(np.float64)
    n = d.size
    return dict(histogram=hist, count=n, underflow=under, overflow=over, nonFinite=int(v.size - n),
                min=float(d.min()) if n else np.nan, max=float(d.max()) if n else np.nan,
                mean=float(d.mean()) if n else np.nan, stddev=float(d.std()) if n else np.nan,
                lo=float(lo), hi=float(hi), binWidth=(float(hi) - float(lo)) / bins)


def raw(values, bins, lo=None, width=None):
    """statistics of decoded raw integers; lo = None: autoRange"""
    x = np.asarray(values, dtype=np.int64).ravel()
    if lo is None:
        lo = int(x.min())
        width = max(1, -(-(int(x.max()) - lo + 1) // bins))
    lo, width = int(lo), int(width)
    under_m = x < lo
    d = (x[~under_m] - lo) // width
    over_m = d >= bins
    hist = np.bincount(d[~over_m], minlength=bins).astype(np.uint64)
    xd = x.astype(np.float64)
    return dict(histogram=hist, count=x.size, underflow=int(under_m.sum()), overflow=int(over_m.sum()), nonFinite=0,
                min=float(xd.min()), max=float(xd.max()), mean=float(xd.mean()), stddev=float(xd.std()),
                lo=float(lo), hi=float(lo + bins * width), binWidth=float(width))


# ------------------------------------------------------------------ raw containers
FORMATS = [(0, 8), (0, 12), (0, 32), (1, 12), (2, 12), (3, 8), (4, 16), (5, 32)]
FORMAT_IDS = ["u8", "u16", "u32", "p12u", "p12s", "i8", "i16", "i32"]


def random_ints(rng, shape, fmt, bit_depth):
    if fmt in (1, 2):
        return rng.integers(0, 4096, size=shape)
    if fmt == 3:
        return rng.integers(-128, 128, size=shape)
    if fmt == 4:
        return rng.integers(-32768, 32768, size=shape)
    if fmt == 5:
        return rng.integers(-2 ** 31, 2 ** 31, size=shape)
    return rng.integers(0, 2 ** min(bit_depth, 32), size=shape, dtype=np.uint64).astype(np.int64)


def encode(ints, fmt, bit_depth):
    """raw bytes (uint8, flat) of integer samples in sample format fmt (OCTPIPE_FORMAT_*), and the decoded integer before bitshift
    (same shape as ints)"""
    if fmt in (1, 2):
        u = (ints.ravel() & 0xFFF).astype(np.uint32)
        s0, s1 = u[0::2], u[1::2]
        b = np.stack([s0 & 0xFF, ((s0 >> 8) & 0xF) | ((s1 & 0xF) << 4), s1 >> 4], axis=-1).astype(np.uint8).ravel()
        dec = u.astype(np.int64) if fmt == 1 else ((u.astype(np.int64) ^ 0x800) - 0x800)
        return b, dec.reshape(ints.shape)
    dt = {3: np.int8, 4: np.int16, 5: np.int32}.get(fmt) or (np.uint8 if bit_depth <= 8 else np.uint16 if bit_depth <= 16 else np.uint32)
    arr = ints.astype(dt)
    return arr.ravel().view(np.uint8), arr.astype(np.int64)


def decoded(dec, fmt, bit_depth, bitshift):
    """the integer the statistics bin: >> 4 under bitshift (arithmetic), except unsigned 32 bit"""
    u32 = fmt == 0 and bit_depth > 16
    return dec if (not bitshift or u32) else (dec >> 4)
