"""Numpy restatement of include/octpipe.h "angiography", written from that comment with plain loops in float64 (no np.var, nothing
vectorised in a way that could change an order).  Volumes are float32 [B][A][L]; a region is (b0, bn, a0, an, s0, sn); a surface is int32
[bn][an] of absolute depth bins, negative = no surface, or None."""
import numpy as np

CANONICAL_NAN = np.uint32(0x7FC00000)
VARIANCE, DECORRELATION, DIFFERENCE = 0, 1, 2


def whole(vol):
    B, A, L = vol.shape
    return (0, B, 0, A, 0, L)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _canonical(x):
    """float32 with a NaN stored as the canonical quiet NaN"""
    x = np.float32(x)
    return CANONICAL_NAN.view(np.float32) if np.isnan(x) else x


_HALF, _ONE = np.float64(0.5), np.float64(1.0)


def _raw_contrast(v, method):
    """(c, mu) in float64 of one bin from its M values as float64 (the caller silences the floating-point warnings)"""
    M = len(v)
    total = v[0]
    for m in range(1, M):
        total = total + v[m]
    mu = total / np.float64(M)
    acc = None
    if method == VARIANCE:
        for m in range(M):
            d = v[m] - mu
            dd = d * d
            acc = dd if acc is None else acc + dd
        return acc / np.float64(M), mu
    for m in range(M - 1):
        if method == DECORRELATION:
            n = v[m] * v[m + 1]
            q = _HALF * (v[m] * v[m]) + _HALF * (v[m + 1] * v[m + 1])
            t = _ONE if q == 0.0 else n / q
        else:
            t = np.abs(v[m + 1] - v[m])
        acc = t if acc is None else acc + t
    avg = acc / np.float64(M - 1)
    return (_ONE - avg if method == DECORRELATION else avg), mu


def bin_contrast(values, method, threshold=None, masked=0.0):
    """(c32 after the mask, mu32 with a NaN canonical) of one bin from its M float32 values"""
    with np.errstate(all="ignore"):
        c, mu = _raw_contrast([np.float64(np.float32(x)) for x in values], method)
        c32, mu32 = _canonical(np.float32(c)), np.float32(mu)
    if threshold is not None and not (mu32 > np.float32(threshold)):  # a strict float32 compare: a NaN mean is masked
        c32 = np.float32(masked)
    return c32, _canonical(mu32)


def apply_mask(out, mean, threshold, masked):
    """the contrast with `masked` wherever !(mean > threshold); per bin, nothing here has an order"""
    res = out.copy()
    with np.errstate(invalid="ignore"):
        res[~(mean > np.float32(threshold))] = np.float32(masked)
    return res


def angiogram(vol, region, repeats, method, threshold=None, masked=0.0):
    """(out, mean), both float32 [P][an][sn]"""
    b0, bn, a0, an, s0, sn = region
    M = int(repeats)
    assert 2 <= M <= 8 and bn % M == 0
    P = bn // M
    out = np.empty((P, an, sn), np.float32)
    mean = np.empty((P, an, sn), np.float32)
    wide = np.asarray(vol, dtype=np.float32).astype(np.float64)  # exact
    nan = CANONICAL_NAN.view(np.float32)
    with np.errstate(all="ignore"):
        for p in range(P):
            for a in range(an):
                rows = [wide[b0 + p * M + m, a0 + a] for m in range(M)]
                for k in range(sn):
                    c, mu = _raw_contrast([row[s0 + k] for row in rows], method)
                    c32, mu32 = np.float32(c), np.float32(mu)
                    out[p, a, k] = nan if c32 != c32 else c32
                    mean[p, a, k] = nan if mu32 != mu32 else mu32
    if threshold is not None:
        out = apply_mask(out, mean, threshold, masked)
    return out, mean


def project(x, function):
    """the en face value of the slab's values x_0, x_1, ... (float32, non-empty)"""
    n = len(x)
    if function == 0:
        with np.errstate(all="ignore"):
            partial = []
            for j in range(min(n, 64)):
                acc = np.float64(x[j])
                for i in range(j + 64, n, 64):
                    acc = acc + np.float64(x[i])
                partial.append(acc)
            total = partial[0]
            for j in range(1, len(partial)):
                total = total + partial[j]
            return _canonical(np.float32(total / np.float64(n)))
    for i in range(n):
        if np.isnan(x[i]):
            return CANONICAL_NAN.view(np.float32)
    for i in range(n):  # the smallest i among those that no other exceeds
        exceeded = False
        for k in range(n):
            if x[k] > x[i]:
                exceeded = True
                break
        if not exceeded:
            return np.float32(x[i])
    raise AssertionError("unreachable")


def project_volume(angio, region, repeats, surface, offset, thickness, function, fill):
    """the en face projection of a contrast volume [P][an][sn] (what angiogram() or the volume call returned for `region`)"""
    b0, bn, a0, an, s0, sn = region
    M = int(repeats)
    P = bn // M
    s1 = s0 + sn - 1
    out = np.empty((P, an), np.float32)
    out.view(np.uint32)[...] = np.float32(fill).view(np.uint32)
    ob, ab = out.view(np.uint32), np.ascontiguousarray(angio, dtype=np.float32)
    for p in range(P):
        for a in range(an):
            s = s0 if surface is None else int(surface[p * M, a])
            if s < 0:
                continue
            lo, hi = max(s + offset, s0), min(s + offset + thickness - 1, s1)
            if lo > hi:
                continue
            x = [ab[p, a, d - s0] for d in range(lo, hi + 1)]
            ob[p, a] = np.float32(project(x, function)).view(np.uint32)
    return out


def angiogram_enface(vol, region, repeats, method, surface, offset, thickness, function, fill, threshold=None, masked=0.0):
    """float32 [P][an]: only the bins of the slabs are worked out"""
    b0, bn, a0, an, s0, sn = region
    M = int(repeats)
    assert 2 <= M <= 8 and bn % M == 0
    P = bn // M
    s1 = s0 + sn - 1
    out = np.empty((P, an), np.float32)
    ob = out.view(np.uint32)
    ob[...] = np.float32(fill).view(np.uint32)
    for p in range(P):
        for a in range(an):
            s = s0 if surface is None else int(surface[p * M, a])
            if s < 0:
                continue
            lo, hi = max(s + offset, s0), min(s + offset + thickness - 1, s1)
            if lo > hi:
                continue
            x = []
            for d in range(lo, hi + 1):
                vals = [vol[b0 + p * M + m, a0 + a, d] for m in range(M)]
                x.append(bin_contrast(vals, method, threshold, masked)[0])
            ob[p, a] = np.float32(project(x, function)).view(np.uint32)
    return out
