"""numpy restatement of the peak analysis definition (include/octpipe.h "peak analysis"), the yardstick of tests/test_peak_analysis.py
and tests/test_gpu_peak_analysis.py.  Everything in float64 on the float32 values, in the order the definition states."""
import math

import numpy as np

NO_PEAK, NONFINITE, WIDTH_UNDEFINED, LEFT_OPEN, RIGHT_OPEN = 1, 2, 4, 8, 16
FIT_CONVERGED, FIT_MAX_ITER, FIT_STALLED, FIT_SKIPPED = 256, 512, 1024, 2048
STEP4_BITS = NO_PEAK | NONFINITE | WIDTH_UNDEFINED | LEFT_OPEN | RIGHT_OPEN
FIT_BITS = FIT_CONVERGED | FIT_MAX_ITER | FIT_STALLED | FIT_SKIPPED
FWHM_PER_SIGMA = 2.3548200450309493  # 2 sqrt(2 ln 2)
CHUNK = 64


def seq_sum(x, axis=0):
    """float64 sum added one after another along axis (np.cumsum is sequential; np.sum is pairwise)"""
    x = np.asarray(x, dtype=np.float64)
    return np.cumsum(x, axis=axis).take(-1, axis=axis)


def averaged(rows):
    """m of one group: rows [G][sampleCount] float32 -> float32 [sampleCount] (chunks of 64, partials in chunk order)"""
    rows = np.asarray(rows, dtype=np.float32)
    g = rows.shape[0]
    parts = np.stack([seq_sum(rows[c:c + CHUNK], axis=0) for c in range(0, g, CHUNK)])
    with np.errstate(invalid="ignore", over="ignore"):
        return (seq_sum(parts, axis=0) / np.float64(g)).astype(np.float32)


def groups_of(region, g):
    """region [bscanCount][ascanCount][sampleCount] -> averaged A-scans [bscanCount][ascanCount // g][sampleCount]"""
    b, a, s = region.shape
    out = np.empty((b, a // g, s), np.float32)
    for i in range(b):
        for j in range(a // g):
            out[i, j] = averaged(region[i, j * g:(j + 1) * g])
    return out


def _empty():
    nan = float("nan")
    return dict(status=0, index=0, value=nan, position=nan, left=nan, right=nan, fwhm=nan, amplitude=nan, center=nan, sigma=nan,
                offset=nan, fitFwhm=nan, rms=nan, fitFirst=0, fitCount=0, iterations=0)


def analyse(m, s0=0, threshold=-np.inf, fit=False, fit_half_width=0, max_iterations=0):
    """steps 1 to 5 on one averaged A-scan m (float32 [sampleCount], depth bins s0 ..): a dict of the OctPipePeak fields"""
    m = np.asarray(m, dtype=np.float32)
    n = len(m)
    o = _empty()
    if not np.all(np.isfinite(m)):
        o["status"] = NONFINITE
        return o
    md = m.astype(np.float64)
    k = int(np.argmax(md))  # the first maximum (no NaN here)
    value = md[k]
    o["index"], o["value"] = s0 + k, float(m[k])
    if not value > float(np.float32(threshold)):
        o["status"] = NO_PEAK
        return o
    status = 0
    position = float(s0 + k)
    if 0 < k < n - 1:
        d = (md[k - 1] - 2.0 * value) + md[k + 1]
        if d < 0.0:
            position = float(s0 + k) + (0.5 * (md[k - 1] - md[k + 1])) / d
    o["position"] = position
    width_ok = value > 0.0
    fwhm = float("nan")
    if not width_ok:
        status |= WIDTH_UNDEFINED
    else:
        half = 0.5 * value
        l = k
        while l > 0 and md[l - 1] > half:
            l -= 1
        if l > 0:
            left = float(s0 + l) - (md[l] - half) / (md[l] - md[l - 1])
        else:
            left = float(s0)
            status |= LEFT_OPEN
        r = k
        while r < n - 1 and md[r + 1] > half:
            r += 1
        if r < n - 1:
            right = float(s0 + r) + (md[r] - half) / (md[r] - md[r + 1])
        else:
            right = float(s0 + n - 1)
            status |= RIGHT_OPEN
        fwhm = right - left
        o["left"], o["right"], o["fwhm"] = left, right, fwhm
    if fit:
        w = int(fit_half_width)
        if not w:
            w = int(min(256.0, max(4.0, math.ceil(1.5 * fwhm)))) if width_ok else 16
        lo, hi = max(0, k - w), min(n - 1, k + w)
        cnt = hi - lo + 1
        o["fitFirst"], o["fitCount"] = s0 + lo, cnt
        if cnt < 5:
            status |= FIT_SKIPPED
        else:
            z = np.arange(s0 + lo, s0 + hi + 1, dtype=np.float64)
            y = md[lo:hi + 1]
            c0 = float(y.min())
            p0 = [value - c0, position, max(0.5, fwhm / FWHM_PER_SIGMA) if width_ok else 1.0, c0]
            p, cost, fst, it = marquardt(z, y, p0, max_iterations or 100)
            status |= fst
            o.update(amplitude=p[0], center=p[1], sigma=abs(p[2]), offset=p[3], fitFwhm=FWHM_PER_SIGMA * abs(p[2]),
                     rms=math.sqrt(cost / cnt), iterations=it)
    o["status"] = status
    return o


def gauss(z, p):
    return p[0] * np.exp(-0.5 * ((z - p[1]) / p[2]) ** 2) + p[3]


def _sums(z, y, p):
    with np.errstate(all="ignore"):
        inv = 1.0 / p[2]
        u = (z - p[1]) * inv
        e = np.exp(-0.5 * (u * u))
        j1 = p[0] * e * u * inv
        J = np.stack([e, j1, j1 * u, np.ones_like(z)], axis=1)
        r = y - (p[0] * e + p[3])
        return J.T @ J, J.T @ r, float(np.sum(r * r))


def solve(H, g, lam):
    """(H + lam diag(H)) delta = g by Gaussian elimination with partial pivoting (the first largest |pivot|); None: a zero or non-finite pivot"""
    M = np.concatenate([H.copy(), g.reshape(4, 1)], axis=1)
    for i in range(4):
        M[i, i] = M[i, i] + lam * M[i, i]
    ok = True
    with np.errstate(all="ignore"):
        for col in range(4):
            piv, best = col, abs(M[col, col])
            for r in range(col + 1, 4):
                if abs(M[r, col]) > best:
                    piv, best = r, abs(M[r, col])
            if piv != col:
                M[[col, piv]] = M[[piv, col]]
            pv = M[col, col]
            if pv == 0.0 or not np.isfinite(pv):
                ok = False
            for r in range(col + 1, 4):
                M[r, col:] -= (M[r, col] / pv) * M[col, col:]
        d = np.zeros(4)
        for i in range(3, -1, -1):
            d[i] = (M[i, 4] - np.dot(M[i, i + 1:4], d[i + 1:4])) / M[i, i]
    return d if ok else None


def marquardt(z, y, p0, max_iterations=100):
    """the definition's Levenberg-Marquardt loop: (parameters, cost, FIT_* bit, solves)"""
    p = np.array(p0, dtype=np.float64)
    H, g, cost = _sums(z, y, p)
    if cost == 0.0:
        return p, cost, FIT_CONVERGED, 0
    lam, it = 1e-3, 0
    while True:
        if it >= max_iterations:
            return p, cost, FIT_MAX_ITER, it
        d = solve(H, g, lam)
        it += 1
        cn = None
        if d is not None:
            pn = p + d
            Hn, gn, cn = _sums(z, y, pn)
        if cn is not None and cn < cost:
            rel = float(np.max(np.abs(d) / (np.abs(p) + 1e-12)))
            conv = cost - cn <= 1e-12 * cost or rel <= 1e-10 or cn == 0.0
            p, H, g, cost = pn, Hn, gn, cn
            lam = max(lam / 10.0, 1e-15)
            if conv:
                return p, cost, FIT_CONVERGED, it
        else:
            lam *= 10.0
            if lam > 1e15:
                return p, cost, FIT_STALLED, it


def analyse_region(region, g, s0=0, **kw):
    """region [bscanCount][ascanCount][sampleCount] float32: (averaged [..][..][sampleCount], list of lists of dicts)"""
    avg = groups_of(region, g)
    return avg, [[analyse(avg[i, j], s0, **kw) for j in range(avg.shape[1])] for i in range(avg.shape[0])]
