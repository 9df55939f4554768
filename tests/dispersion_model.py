"""float64 model of the dispersion sweep (include/octpipe.h "dispersion estimation"), shared by test_dispersion_sweep.py (CPU)
and test_gpu_dispersion_sweep.py.

Values: the oracle's stages (oracle/octref.py: unpack, rolling_average, klin with the candidate's phasor, idft), |z| and the
grey-value mapping in float64.  Bounds: the suite's frozen per-bin amplitude policy (common.amp_rtol: | |Z_got| - |Z_want| | <=
amp_rtol(N) x the A-scan's largest amplitude) carried through the value mapping, plus one unit in the last place of the float32 value
(the resolution of the number the kernel stores).  The metric bounds follow from the per-bin bounds; the sums add the float32
rounding of the kernel's summation (N/128 sequential terms per lane, a 6-level butterfly)."""
import numpy as np

import common
from oracle import octref

SUM, SAMPLES, PEAK, SOBEL = 0, 1, 2, 3
METRICS = (SUM, SAMPLES, PEAK, SOBEL)


def grey_scaling(p, n, linear):
    """sA, sB of value = sA * s + sB, s = sqrt(P) (linear) or log2(P) (log): the float64 constants of octpipe_api.hip"""
    half, rng = n / 2.0, float(p.signalGrayscaleMax) - float(p.signalGrayscaleMin)
    coeff, addend, mn = float(p.signalMultiplicator), float(p.signalAddend), float(p.signalGrayscaleMin)
    if linear:
        return coeff / (half * rng), coeff * (-mn / rng + addend)
    return coeff * 10.0 * np.log10(2.0) / rng, coeff * ((-10.0 * np.log10(half) - mn) / rng + addend)


def values_from_power(P, p, n, linear):
    sA, sB = grey_scaling(p, n, linear)
    with np.errstate(divide="ignore"):
        s = np.sqrt(P) if linear else np.log2(P)
    return sA * s + sB


def per_bin_bound(P, p, n, linear):
    """[M, N/2] bound of |value_kernel - value_model| from the amplitude policy; inf where the amplitude bound reaches zero (log)"""
    amp = np.sqrt(P)
    delta = common.amp_rtol(n) * amp.max(axis=1, keepdims=True)
    sA, _ = grey_scaling(p, n, linear)
    v = values_from_power(P, p, n, linear)
    if linear:
        b = np.abs(sA) * np.broadcast_to(delta, amp.shape)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            b = np.where(amp > delta, np.abs(sA) * np.log2(amp / np.maximum(amp - delta, 1e-300)) * 2.0, np.inf)
    with np.errstate(invalid="ignore"):
        ulp = np.where(np.isfinite(v), np.spacing(np.abs(v).astype(np.float32)).astype(np.float64), 0.0)
    return b + ulp


def model_power(raw, p, d0, d1, d2, d3, first, count):
    """|z|^2 [count, N/2] of A-scans first .. first+count-1 under the handle's settings with candidate (d2, d3) applied, FPN / background /
    flip / sinusoidal correction off"""
    n = int(p.samplesPerLine)
    lines = int(p.ascansPerBscan) * int(p.bscansPerBuffer)
    x = octref.unpack(raw, int(p.bitDepth), int(p.bitshift))
    if p.backgroundRemoval and p.rollingAverageWindowSize > 0:
        x = octref.rolling_average(x, int(p.rollingAverageWindowSize), n, lines)
    phase = octref.dispersive_phase(octref.dispersion_curve([d0, d1, d2, d3], n))
    window = p.windowCurve if p.windowing else None
    if p.resampling:
        x = octref.klin(x, int(p.resamplingInterpolation), p.resampleCurve, window, phase)
    else:  # linear interpolation at integer positions: the sample itself
        x = octref.klin(x, 0, np.arange(n, dtype=np.float32), window, phase)
    z = octref.idft(x[first * n:(first + count) * n], n).reshape(count, n)[:, :n // 2].astype(np.complex128)
    return z.real ** 2 + z.imag ** 2


def metric(v, kind, threshold, ignore):
    """per-A-scan metric of values v [M, N/2] (float64, vectorised)"""
    v = np.asarray(v, dtype=np.float64)
    half = v.shape[1]
    w = v[:, ignore:]
    if kind == SUM:
        return np.where(w > threshold, w, 0.0).sum(axis=1)
    if kind == SAMPLES:
        return (w > threshold).sum(axis=1).astype(np.float64)
    if kind == PEAK:
        return w.max(axis=1)
    k = np.arange(ignore + 1, half - 1)
    return np.abs(v[:, k + 1] - v[:, k - 1]).sum(axis=1)


def metric_naive(v, kind, threshold, ignore):
    """the same, one bin at a time (the specification's wording)"""
    out = []
    for row in np.asarray(v, dtype=np.float64):
        half = len(row)
        if kind == SOBEL:
            acc = 0.0
            for k in range(ignore + 1, half - 2 + 1):
                acc += abs(row[k + 1] - row[k - 1])
            out.append(acc)
            continue
        acc, cnt, best = 0.0, 0, -np.inf
        for k in range(ignore, half):
            if row[k] > threshold:
                acc += row[k]
                cnt += 1
            best = max(best, row[k])
        out.append({SUM: acc, SAMPLES: float(cnt), PEAK: best}[kind])
    return np.array(out)


def metric_bound(v, b, kind, threshold, ignore):
    """per-A-scan bound of |metric_kernel - metric_model| given per-bin bounds b (SAMPLES: the number of bins within their bound of the
    threshold, where the count may legitimately differ)"""
    v, b = np.asarray(v, dtype=np.float64), np.asarray(b, dtype=np.float64)
    half = v.shape[1]
    gamma = (half / 64.0 + 8.0) * 2.0 ** -24  # float32 summation: N/128 terms per lane, 6 butterfly levels (+ margin of two)
    w, bw = v[:, ignore:], b[:, ignore:]
    if kind == PEAK:
        return bw.max(axis=1) + np.spacing(np.abs(w).max(axis=1).astype(np.float32))
    ambiguous = np.abs(w - threshold) <= bw
    if kind == SAMPLES:
        return ambiguous.sum(axis=1).astype(np.float64)
    if kind == SUM:
        inside = (w > threshold) & ~ambiguous
        terms = np.where(inside, bw, 0.0) + np.where(ambiguous, np.abs(w) + bw, 0.0)
        return terms.sum(axis=1) + gamma * (np.abs(w) + bw).sum(axis=1)
    k = np.arange(ignore + 1, half - 1)
    d = np.abs(v[:, k + 1] - v[:, k - 1])
    return (b[:, k + 1] + b[:, k - 1]).sum(axis=1) + gamma * (d + b[:, k + 1] + b[:, k - 1]).sum(axis=1) + np.spacing(d.astype(np.float32)).sum(axis=1)


def layered_raw(p, d2_true=0.0, d3_true=0.0, seed=5, reflectors=((0.09, 350.0), (0.17, 250.0), (0.31, 300.0)), noise=4.0, dc=1800.0):
    """uint16 raw buffer of a layered sample (DC, several reflectors, noise) whose fringes carry the dispersion phase of (d2_true, d3_true)
    on top of the handle's d0 / d1: compensating with exactly that candidate makes every reflector a sharp peak.  Resampling off."""
    n, lines = int(p.samplesPerLine), int(p.ascansPerBscan) * int(p.bscansPerBuffer)
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.float64)
    theta = octref.dispersion_curve([float(p.d0), float(p.d1), float(d2_true), float(d3_true)], n).astype(np.float64)
    sig = np.full(n, dc)
    for z, a in reflectors:
        # the kernel multiplies by e^{+i theta} and transforms with e^{+2 pi i j k / N}: a fringe e^{-i (2 pi kz j / N + theta)}
        # lands at depth bin kz once theta is compensated.  kz is a whole bin: a reflector between two bins would make a residual phase
        # with a linear part (a shift onto the bin) look sharper than the exact compensation
        kz = round(z * n)
        sig = sig + a * np.cos(2.0 * np.pi * kz * j / n + theta)
    out = sig[None, :] + rng.normal(0.0, noise, size=(lines, n))
    return np.clip(np.rint(out), 0, 4095).astype(np.uint16)
