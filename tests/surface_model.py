"""Numpy restatement of include/octpipe.h "surface views", written from that comment with plain loops (no vectorised shortcuts that
could share a mistake with the kernels).  Volumes are float32 [B][A][L]; a region is (b0, bn, a0, an, s0, sn); surfaces are int32
[bn][an] of absolute depth bins, negative = no surface."""
import numpy as np

CANONICAL_NAN = np.uint32(0x7FC00000)


def whole(vol):
    B, A, L = vol.shape
    return (0, B, 0, A, 0, L)


def _rows(vol, region):
    b0, bn, a0, an, s0, sn = region
    for b in range(bn):
        for a in range(an):
            yield b, a, vol[b0 + b, a0 + a]


def detect(vol, region, threshold, run):
    b0, bn, a0, an, s0, sn = region
    s1 = s0 + sn - 1
    thr = np.float32(threshold)
    out = np.full((bn, an), -1, np.int32)
    for b, a, v in _rows(vol, region):
        for d in range(s0, s1 - run + 2):
            ok = True
            for i in range(run):
                if not (v[d + i] > thr):  # strict float32 compare: NaN never exceeds
                    ok = False
                    break
            if ok:
                out[b, a] = d
                break
    return out


def smooth(surface, radius):
    rows, cols = surface.shape
    out = np.full((rows, cols), -1, np.int32)
    for r in range(rows):
        for c in range(cols):
            vals = []
            for rr in range(max(0, r - radius), min(rows, r + radius + 1)):
                for cc in range(max(0, c - radius), min(cols, c + radius + 1)):
                    if surface[rr, cc] >= 0:
                        vals.append(int(surface[rr, cc]))
            if vals:
                vals.sort()
                out[r, c] = vals[(len(vals) - 1) // 2]
    return out


def _canonical(x):
    """float32 with a NaN stored as the canonical quiet NaN"""
    x = np.float32(x)
    return CANONICAL_NAN.view(np.float32) if np.isnan(x) else x


def slab(v, lo, hi, function):
    """the en face value of bins lo .. hi (inclusive, non-empty) of one A-scan"""
    if function == 0:
        with np.errstate(all="ignore"):
            acc = np.float64(v[lo])
            for d in range(lo + 1, hi + 1):
                acc = acc + np.float64(v[d])
            return _canonical(np.float32(acc / np.float64(hi - lo + 1)))
    nan = False
    m = v[lo]
    for d in range(lo, hi + 1):
        nan = nan or bool(np.isnan(v[d]))
        if v[d] > m:
            m = v[d]
    return CANONICAL_NAN.view(np.float32) if nan else np.float32(m)


def enface(vol, region, surface, offset, thickness, function, fill):
    b0, bn, a0, an, s0, sn = region
    s1 = s0 + sn - 1
    out = np.empty((bn, an), np.float32)
    out[...] = np.float32(fill)
    for b, a, v in _rows(vol, region):
        s = int(surface[b, a])
        if s < 0:
            continue
        lo, hi = max(s + offset, s0), min(s + offset + thickness - 1, s1)
        if lo <= hi:
            out[b, a] = slab(v, lo, hi, function)
    return out


def flatten(vol, region, surface, anchor, out_depth, fill):
    b0, bn, a0, an, s0, sn = region
    s1 = s0 + sn - 1
    out = np.empty((bn, an, out_depth), np.float32)
    out[...] = np.float32(fill)
    bits, src = out.view(np.uint32), np.ascontiguousarray(vol).view(np.uint32)
    for b in range(bn):
        for a in range(an):
            s = int(surface[b, a])
            if s < 0:
                continue
            for j in range(out_depth):
                k = s - anchor + j
                if s0 <= k <= s1:
                    bits[b, a, j] = src[b0 + b, a0 + a, k]  # the bits are copied
    return out


def fixed_slab(flat, first, thickness, function, fill):
    """the fixed-depth slab of a flattened volume: rows first .. first + thickness - 1 as far as they exist, per A-scan; `fill` for none"""
    bn, an, depth = flat.shape
    out = np.empty((bn, an), np.float32)
    out[...] = np.float32(fill)
    lo, hi = max(first, 0), min(first + thickness - 1, depth - 1)
    if lo <= hi:
        for b in range(bn):
            for a in range(an):
                out[b, a] = slab(flat[b, a], lo, hi, function)
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
