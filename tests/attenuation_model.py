"""Numpy restatement of include/octpipe.h "attenuation", written from that comment: float64 throughout, every product an array operation
of its own (numpy never fuses a multiply with an add), vectorised over A-scans -- the lanes of the definition are an array axis, its
steps are statements.  Volumes are float32 [B][A][L]; a region is (b0, bn, a0, an, s0, sn); a surface is int32 [bn][an] of absolute
depth bins, negative = no surface.  Scales: INTENSITY, AMPLITUDE, LOG2."""
import math

import numpy as np

import surface_model as sm

INTENSITY, AMPLITUDE, LOG2 = 0, 1, 2
CHUNK, LANES, PIECE = 256, 64, 4
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
COEFF = [1.0 / math.factorial(k) for k in range(14)]  # the doubles nearest 1 / k!: one correctly rounded division each
CANONICAL_NAN = np.uint32(0x7FC00000)


def whole(vol):
    return sm.whole(vol)


def bits(x):
    return sm.bits(x)


def pow2(y):
    """2 ** y as the definition has it"""
    y = np.asarray(y, np.float64)
    inside = (y >= -1000.0) & (y < 1024.0)  # (False for NaN)
    yc = np.where(inside, y, 0.0)
    m = np.rint(yc)
    f = yc - m
    t = f * LN2
    p = np.full_like(t, COEFF[13])
    for k in range(12, -1, -1):
        tp = t * p
        p = COEFF[k] + tp
    r = np.ldexp(p, m.astype(np.int32))
    outside = np.where(y >= 1024.0, np.inf, np.where(y < -1000.0, 0.0, np.nan))
    return np.where(inside, r, outside)


def intensity(v, scale=INTENSITY, a=1.0, b=0.0, noise=0.0, gain=None):
    """I of every bin: v float32 [..., n], gain float32 [n] or None; float64 [..., n]"""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        xv = v.astype(np.float64) * np.float64(a)
        x = xv + np.float64(b)
        if scale == INTENSITY:
            J = x
        elif scale == AMPLITUDE:
            J = x * x
        else:
            J = pow2(x)
        K = J - np.float64(np.float32(noise))
        L = K if gain is None else K * np.asarray(gain, np.float32).astype(np.float64)
        return np.where(L > 0.0, L, 0.0)  # NaN and negatives: +0


def below_sums(I, tail=0.0):
    """the sum below every bin in the defined order: I float64 [rows][n] -> float64 [rows][n]"""
    I = np.asarray(I, np.float64)
    rows, n = I.shape
    chunks = (n + CHUNK - 1) // CHUNK
    padded = np.zeros((rows, chunks * CHUNK), np.float64)  # bins >= n count as +0
    padded[:, :n] = I
    q = padded.reshape(rows, chunks, LANES, PIECE)
    below = np.empty_like(q)
    C = np.full(rows, np.float64(np.float32(tail)))
    with np.errstate(all="ignore"):
        for k in range(chunks - 1, -1, -1):
            i0, i1, i2, i3 = (q[:, k, :, j] for j in range(PIECE))
            t = ((i3 + i2) + i1) + i0  # Q_l
            for s in (1, 2, 4, 8, 16, 32):
                step = t.copy()  # all lanes at once from the previous step's values
                step[:, :LANES - s] = t[:, :LANES - s] + t[:, s:]
                t = step
            R = np.empty_like(t)
            R[:, LANES - 1] = C
            R[:, :LANES - 1] = t[:, 1:] + C[:, None]
            below[:, k, :, 3] = R
            below[:, k, :, 2] = below[:, k, :, 3] + i3
            below[:, k, :, 1] = below[:, k, :, 2] + i2
            below[:, k, :, 0] = below[:, k, :, 1] + i1
            C = t[:, 0] + C
    return np.ascontiguousarray(below.reshape(rows, chunks * CHUNK)[:, :n])


def running_sums(I, tail=0.0):
    """NOT the definition: one running sum from the deep end (what the defined order is told apart from)"""
    I = np.asarray(I, np.float64)
    out = np.empty_like(I)
    acc = np.full(I.shape[0], np.float64(np.float32(tail)))
    with np.errstate(all="ignore"):
        for i in range(I.shape[1] - 1, -1, -1):
            out[:, i] = acc
            acc = acc + I[:, i]
    return out


def coefficient(I, below, pixel_size, undefined=np.nan):
    """mu32 of every bin, float32 with the bits the definition gives"""
    with np.errstate(all="ignore"):
        den = (2.0 * np.float64(np.float32(pixel_size))) * below
        mu = (I / den).astype(np.float32)
    out = mu.view(np.uint32).copy()
    out[np.isnan(mu)] = CANONICAL_NAN
    out[~(den > 0.0)] = np.asarray(undefined, np.float32).reshape(1).view(np.uint32)[0]  # its bits as given
    return out.view(np.float32)


def _window(vol, region):
    b0, bn, a0, an, s0, sn = region
    return np.ascontiguousarray(np.asarray(vol, np.float32)[b0:b0 + bn, a0:a0 + an, s0:s0 + sn]).reshape(bn * an, sn)


def sums(vol, region, scale=INTENSITY, a=1.0, b=0.0, noise=0.0, tail=0.0, gain=None):
    """float64 [bn][an][sn]: what octpipe_debug_attenuation_sums writes"""
    b0, bn, a0, an, s0, sn = region
    return below_sums(intensity(_window(vol, region), scale, a, b, noise, gain), tail).reshape(bn, an, sn)


def attenuation(vol, region, pixel_size, scale=INTENSITY, a=1.0, b=0.0, noise=0.0, tail=0.0, gain=None, undefined=np.nan):
    """float32 [bn][an][sn]: what octpipe_attenuation writes"""
    b0, bn, a0, an, s0, sn = region
    I = intensity(_window(vol, region), scale, a, b, noise, gain)
    return coefficient(I, below_sums(I, tail), pixel_size, undefined).reshape(bn, an, sn)


def attenuation_enface(vol, region, pixel_size, surface=None, offset=0, thickness=1, function=0, fill=0.0, scale=INTENSITY, a=1.0, b=0.0,
                       noise=0.0, tail=0.0, gain=None, undefined=np.nan):
    """float32 [bn][an]: the surface views' en face of the volume attenuation() gives for the same region (surface None: firstSample)"""
    b0, bn, a0, an, s0, sn = region
    vol = np.asarray(vol, np.float32)
    mu = np.zeros(vol.shape, np.float32)  # (only the region's window is ever read)
    mu[b0:b0 + bn, a0:a0 + an, s0:s0 + sn] = attenuation(vol, region, pixel_size, scale, a, b, noise, tail, gain, undefined)
    if surface is None:
        surface = np.full((bn, an), s0, np.int32)
    return sm.enface(mu, region, surface, offset, thickness, function, fill)
