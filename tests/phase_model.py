"""Float64 model of the phase extraction (include/octpipe.h "phase extraction", item 3) and the synthetic calibration data the tests use.

The calibration fringe is sampled non-linearly in k: sample n sits at k(u), u = n / (N-1), with the monotone map
k(u) = u + 0.15 u (1-u) + 0.1 u (1-u) (u - 0.5).  A fringe cos(2 pi f0 (N-1) k(u) / N) then has the phase theta(n) = 2 pi f0 (N-1) k(u_n) / N,
so the normalised phase is psi_true(n) = a + (k(u_n) - k(u_a)) (b - a) / (k(u_b) - k(u_a)) and the analytic curve is its inverse."""
import numpy as np


def k_map(u, c2=0.15, c3=0.1):
    return u + c2 * u * (1.0 - u) + c3 * u * (1.0 - u) * (u - 0.5)


def calibration_raw(n, lines, seed=1, f0=None, amp=600.0, sample_amp=120.0, noise=6.0, kmap=k_map, dtype=np.uint16):
    """[lines, n] 12-bit raw calibration A-scans: the mirror fringe at f0 bins plus weaker sample reflectors that differ per A-scan
    (averaging suppresses them) and integer noise"""
    rng = np.random.default_rng(seed)
    f0 = 0.3 * n if f0 is None else f0
    u = np.arange(n, dtype=np.float64) / (n - 1)
    k = kmap(u)
    sig = 2048.0 + amp * np.cos(2.0 * np.pi * f0 * (n - 1) * k / n)
    out = np.empty((lines, n), dtype=np.float64)
    for i in range(lines):
        row = sig.copy()
        for _ in range(3):
            d = rng.uniform(0.03, 0.45) * n
            row += sample_amp * rng.uniform(0.2, 1.0) * np.cos(2.0 * np.pi * d * (n - 1) * k / n + rng.uniform(0, 2 * np.pi))
        out[i] = row
    out += rng.integers(-int(noise), int(noise) + 1, size=out.shape)
    return np.clip(np.rint(out), 0, 4095).astype(dtype)


def psi_true(n, a, b, kmap=k_map):
    u = np.arange(n, dtype=np.float64) / (n - 1)
    k = kmap(u)
    return a + (k - k[a]) * (b - a) / (k[b] - k[a])


def analytic_curve(n, a, b, kmap=k_map, iters=60):
    """curve[j] = psi_true^{-1}(j) on the continuous axis, by bisection in float64 (psi_true is strictly increasing)"""
    ka, kb = kmap(a / (n - 1.0)), kmap(b / (n - 1.0))
    j = np.arange(n, dtype=np.float64)
    target = ka + (j - a) * (kb - ka) / (b - a)  # k(u(curve[j])) = target
    lo, hi = np.full(n, -0.5), np.full(n, n - 0.5)
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        below = kmap(mid / (n - 1.0)) < target
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    return 0.5 * (lo + hi)


def _transform(x, inverse, transform_dtype):
    """np.fft of x in float64, or, transform_dtype = np.complex64, in single precision (numpy >= 2 keeps complex64; an older numpy
    widens it, then torch.fft on the CPU does the same transform) -- returned as complex128 either way"""
    if np.dtype(transform_dtype) != np.dtype(np.complex64):
        return np.fft.ifft(x) if inverse else np.fft.fft(x)
    x32 = np.asarray(x).astype(np.complex64)
    y = np.fft.ifft(x32) if inverse else np.fft.fft(x32)
    if y.dtype != np.complex64:
        import torch
        t = torch.from_numpy(x32)
        y = (torch.fft.ifft(t) if inverse else torch.fft.fft(t)).numpy()
    assert y.dtype == np.complex64
    return y.astype(np.complex128)


def extract(mean, peak_start, peak_end, window_raw=False, hann_peak=True, ignore_first=0, ignore_last=0, transform_dtype=np.float64):
    """The library's definition, step by step in float64: dict of spectrum, envelope, phase, psi, psi_mono, curve, coeffs.
    transform_dtype = np.complex64 runs the two transforms (and the band window's product) in single precision, as the device does;
    everything behind them stays float64."""
    single = np.dtype(transform_dtype) == np.dtype(np.complex64)
    m = np.asarray(mean, dtype=np.float64)
    n = len(m)
    a, b = int(ignore_first), n - 1 - int(ignore_last)
    s, e = int(peak_start), int(peak_end)
    x = m - m.sum() / n
    idx = np.arange(n, dtype=np.float64)
    if window_raw:
        x = x * (0.5 - 0.5 * np.cos(2.0 * np.pi * idx / (n - 1)))
    X = _transform(x, False, transform_dtype)
    w = np.zeros(n)
    kk = np.arange(s, e + 1, dtype=np.float64)
    w[s:e + 1] = 0.5 - 0.5 * np.cos(2.0 * np.pi * (kk - s) / (e - s)) if hann_peak else 1.0
    z = _transform((w.astype(np.float32) * X.astype(np.complex64)) if single else w * X, True, transform_dtype)
    env = np.abs(z)
    pw = np.arctan2(z.imag, z.real)
    d = np.diff(pw)
    J = np.concatenate([[0], np.where(d > np.pi, -1, np.where(d < -np.pi, 1, 0))])
    K = np.cumsum(J)
    phi = pw - pw[a] + 2.0 * np.pi * (K - K[a])
    if phi[b] == 0.0 or not np.isfinite(phi[b]):
        raise ValueError("no calibration signal in the selected band")
    psi = a + phi * ((b - a) / phi[b])
    mono = psi.copy()
    mono[a:] = np.maximum.accumulate(psi[a:])
    mono[:a + 1] = np.minimum.accumulate(psi[:a + 1][::-1])[::-1]
    curve = invert(mono)
    return dict(spectrum=np.abs(X[:n // 2]), envelope=env, phase=phi, psi=psi, psi_mono=mono, curve=curve,
                coeffs=fit_cubic(curve, a, b), a=a, b=b)


def forward(mono, c):
    """the piecewise-linear psi_mono at the fractional positions c"""
    mono = np.asarray(mono, np.float64)
    c = np.asarray(c, np.float64)
    n = len(mono)
    i = np.clip(np.floor(c).astype(np.int64), 0, n - 2)
    return mono[i] + (c - i) * (mono[i + 1] - mono[i])


def invert(mono):
    n = len(mono)
    j = np.arange(n, dtype=np.float64)
    ns = np.searchsorted(mono[:n - 1], j, side="right") - 1  # largest n <= N-2 with psi(n) <= j
    ns = np.clip(ns, 0, n - 2)
    with np.errstate(divide="ignore", invalid="ignore"):  # (flat steps only where the clamps below take over)
        c = ns + (j - mono[ns]) / (mono[ns + 1] - mono[ns])
    c = np.where(j < mono[0], 0.0, c)
    return np.where(j >= mono[n - 1], float(n - 1), c)


def fit_cubic(curve, a, b):
    """least squares of curve[j], j in [a, b], on {1, t, t^2, t^3}, t = j / (N-1): the normal equations in exact rational arithmetic,
    rounded once at the end.  (float64 lstsq on the powers of t is good to about cond x eps: fine for a wide [a, b], off by 7e-2 in
    c0 for 11 samples next to N-1 = 4095, where the condition of the powers of t is 2.6e10.)"""
    from fractions import Fraction
    n = len(curve)
    y = np.asarray(curve, np.float64)
    # in s = 2 j - (a + b), an integer: sums of s^k exactly, then s = 2 (n-1) t - (a + b)
    M = [[Fraction(0)] * 5 for _ in range(4)]
    pw = [0] * 7
    rhs = [Fraction(0)] * 4
    for j in range(a, b + 1):
        s = 2 * j - (a + b)
        for k in range(7):
            pw[k] += s ** k
        yj = Fraction(float(y[j]))
        for k in range(4):
            rhs[k] += yj * s ** k
    for r in range(4):
        for c in range(4):
            M[r][c] = Fraction(pw[r + c])
        M[r][4] = rhs[r]
    for c in range(4):
        piv = next(r for r in range(c, 4) if M[r][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        for r in range(c + 1, 4):
            f = M[r][c] / M[c][c]
            M[r] = [x - f * z for x, z in zip(M[r], M[c])]
    d = [Fraction(0)] * 4
    for r in range(3, -1, -1):
        d[r] = (M[r][4] - sum(M[r][k] * d[k] for k in range(r + 1, 4))) / M[r][r]
    alpha, beta = Fraction(2 * (n - 1)), Fraction(-(a + b))
    binom = [[1], [1, 1], [1, 2, 1], [1, 3, 3, 1]]
    out = [Fraction(0)] * 4
    for k in range(4):
        for i in range(k + 1):
            out[i] += d[k] * binom[k][i] * alpha ** i * beta ** (k - i)
    return np.array([float(v) for v in out])


def poly_curve(coeffs, n):
    t = np.arange(n, dtype=np.float64) / (n - 1)
    return coeffs[0] + coeffs[1] * t + coeffs[2] * t * t + coeffs[3] * t ** 3


# ------------------------------------------------------------------ imaging check
def mirror(n, depth, kmap=k_map):
    u = np.arange(n, dtype=np.float64) / (n - 1)
    return np.cos(2.0 * np.pi * depth * (n - 1) * kmap(u) / n)


def resample_cubic(y, curve):
    """Catmull-Rom interpolation of y at the fractional positions curve (clamped to the row like the product's curve clamp)"""
    n = len(y)
    c = np.clip(np.asarray(curve, np.float64), 0.0, n - 3.0)
    i = np.floor(c).astype(int)
    t = c - i
    p0, p1, p2, p3 = y[np.abs(i - 1)], y[i], y[i + 1], y[i + 2]
    return p1 + 0.5 * t * (p2 - p0 + t * (2 * p0 - 5 * p1 + 4 * p2 - p3 + t * (3 * (p1 - p2) + p3 - p0)))


def ascan(y):
    n = len(y)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))
    return np.abs(np.fft.fft((y - y.mean()) * w))[:n // 2]


def peak_and_fwhm(a, skip=8):
    """height of the highest bin beyond `skip` and its full width at half maximum in bins (linear interpolation on both flanks)"""
    k = skip + int(np.argmax(a[skip:]))
    h = a[k]
    half = 0.5 * h
    l = k
    while l > 0 and a[l - 1] > half:
        l -= 1
    r = k
    while r < len(a) - 1 and a[r + 1] > half:
        r += 1
    left = l - (a[l] - half) / (a[l] - a[l - 1]) if l > 0 else float(l)
    right = r + (a[r] - half) / (a[r] - a[r + 1]) if r < len(a) - 1 else float(r)
    return h, right - left
