"""Numpy restatement of include/octpipe.h "repeat registration", written from that comment in float64 with the stated order of additions:
every sum below is a Python loop of element-wise adds (over independent groups, lags or partials at once), never np.sum or any other
reduction whose order numpy chooses.  Volumes are float32 [B][A][L]; a region is (b0, bn, a0, an, s0, sn); shifts are int32 [P][M][Qp]."""
import numpy as np

import angio_model as am

CANONICAL_NAN = am.CANONICAL_NAN
CANONICAL_NAN64 = np.uint64(0x7FF8000000000000)
CHUNK = 64


def averaged(rows):
    """the peak analysis' averaged A-scan of G rows [G][...][sn] (float32): chunks of 64 rows, float64 partials in row order, the partials in
    chunk order, (float)(T / G)"""
    rows = np.asarray(rows, dtype=np.float32)
    G = rows.shape[0]
    with np.errstate(all="ignore"):
        total = None
        for c0 in range(0, G, CHUNK):
            part = rows[c0].astype(np.float64)
            for i in range(c0 + 1, min(G, c0 + CHUNK)):
                part = part + rows[i].astype(np.float64)
            total = part if total is None else total + part
        return (total / np.float64(G)).astype(np.float32)


def profiles(vol, region, repeats, G):
    """float32 [P][M][Qp][sn]: P_m of every group"""
    b0, bn, a0, an, s0, sn = region
    M = int(repeats)
    assert 2 <= M <= 8 and bn % M == 0 and G >= 1 and an % G == 0
    P, Qp = bn // M, an // G
    cut = np.asarray(vol, dtype=np.float32)[b0:b0 + bn, a0:a0 + an, s0:s0 + sn].reshape(P, M, Qp, G, sn)
    return averaged(np.moveaxis(cut, 3, 0))


def lag_costs(p0, pm, R):
    """C(d) for d = -R ... R, float64 [...][2R + 1], of the profiles p0 and pm [...][sn] (finite float32)"""
    p0, pm = np.asarray(p0, dtype=np.float32).astype(np.float64), np.asarray(pm, dtype=np.float32).astype(np.float64)
    sn = p0.shape[-1]
    K = sn - 2 * R
    assert 1 <= R <= 64 and K >= 1
    out = np.empty(p0.shape[:-1] + (2 * R + 1,), np.float64)
    with np.errstate(all="ignore"):
        for d in range(-R, R + 1):
            t = np.abs(pm[..., R + d:R + d + K] - p0[..., R:R + K])  # t_i, i = 0 ... K - 1
            part = t[..., :min(K, 64)].copy()  # L_j starts from t_j
            for i0 in range(64, K, 64):
                w = min(64, K - i0)
                part[..., :w] = part[..., :w] + t[..., i0:i0 + w]
            c = part[..., 0]
            for j in range(1, part.shape[-1]):
                c = c + part[..., j]
            out[..., d + R] = c
    return out


def pick(costs, R):
    """the lag with the smallest cost; among equal costs the smallest |d|, then the negative one (costs [2R + 1], finite)"""
    best = None
    for d in sorted(range(-R, R + 1), key=lambda d: (abs(d), d)):
        c = costs[d + R]
        if best is None or c < best[0]:
            best = (c, d)
    return best[1]


def repeat_shifts(vol, region, repeats, G=None, R=8):
    """(shifts int32 [P][M][Qp], costs float64 [P][M - 1][Qp][2R + 1], profiles float32 [P][M][Qp][sn])"""
    b0, bn, a0, an, s0, sn = region
    G = an if G is None else int(G)
    prof = profiles(vol, region, repeats, G)
    P, M, Qp, _ = prof.shape
    shifts = np.zeros((P, M, Qp), np.int32)
    costs = np.empty((P, M - 1, Qp, 2 * R + 1), np.float64)
    finite = np.isfinite(prof).all(axis=-1)  # [P][M][Qp]
    for m in range(1, M):
        c = lag_costs(np.nan_to_num(prof[:, 0]), np.nan_to_num(prof[:, m]), R)  # (the groups with a non-finite value are overwritten below)
        for p in range(P):
            for j in range(Qp):
                if finite[p, 0, j] and finite[p, m, j]:
                    shifts[p, m, j] = pick(c[p, j], R)
                else:
                    c[p, j].view(np.uint64)[...] = CANONICAL_NAN64
        costs[:, m - 1] = c
    return shifts, costs, prof


def covered(shifts_of_group, s0, sn):
    """(lo, hi): the bins of W inside Wc, absolute; lo > hi: none.  Python integers: no overflow"""
    d = [int(x) for x in shifts_of_group]
    return max(s0, s0 + max(-x for x in d)), min(s0 + sn - 1, s0 + sn - 1 - max(d))


def _fill_bits(shape, fill):
    out = np.empty(shape, np.float32)
    out.view(np.uint32)[...] = np.float32(fill).view(np.uint32)
    return out


def angiogram_registered(vol, region, repeats, method, shifts, G=None, fill=0.0, threshold=None, masked=0.0):
    """(out, mean), both float32 [P][an][sn]: the angiography's contrast of the shifted bins inside Wc, `fill` outside"""
    b0, bn, a0, an, s0, sn = region
    M = int(repeats)
    G = an if G is None else int(G)
    P, Qp = bn // M, an // G
    shifts = np.asarray(shifts).reshape(P, M, Qp)
    out, mean = _fill_bits((P, an, sn), fill), _fill_bits((P, an, sn), fill)
    vol = np.asarray(vol, dtype=np.float32)
    for p in range(P):
        for a in range(an):
            d = [int(x) for x in shifts[p, :, a // G]]
            lo, hi = covered(d, s0, sn)
            if lo > hi:
                continue
            # the shifted bins as a volume of their own: [M][1][hi - lo + 1], then the angiography section on it
            moved = np.stack([vol[b0 + p * M + m, a0 + a, lo + d[m]:hi + d[m] + 1] for m in range(M)])[:, None, :]
            assert moved.shape[2] == hi - lo + 1
            o, mu = am.angiogram(moved, am.whole(moved), M, method, threshold, masked)
            out[p, a, lo - s0:hi - s0 + 1] = o[0, 0]
            mean[p, a, lo - s0:hi - s0 + 1] = mu[0, 0]
    return out, mean


def angiogram_enface_registered(vol, region, repeats, method, shifts, G, surface, offset, thickness, function, fill, threshold=None, masked=0.0):
    """float32 [P][an]: the slab's bins inside W and Wc, projected as the angiography section says"""
    b0, bn, a0, an, s0, sn = region
    M = int(repeats)
    G = an if G is None else int(G)
    P, Qp = bn // M, an // G
    shifts = np.asarray(shifts).reshape(P, M, Qp)
    out = _fill_bits((P, an), fill)
    ob = out.view(np.uint32)
    for p in range(P):
        for a in range(an):
            s = s0 if surface is None else int(surface[p * M, a])
            if s < 0:
                continue
            d = [int(x) for x in shifts[p, :, a // G]]
            clo, chi = covered(d, s0, sn)
            lo, hi = max(s + offset, clo), min(s + offset + thickness - 1, chi)
            if lo > hi:
                continue
            x = []
            for k in range(lo, hi + 1):
                vals = [vol[b0 + p * M + m, a0 + a, k + d[m]] for m in range(M)]
                x.append(am.bin_contrast(vals, method, threshold, masked)[0])
            ob[p, a] = np.float32(am.project(x, function)).view(np.uint32)
    return out


def project_registered(angio, region, repeats, shifts, G, surface, offset, thickness, function, fill):
    """the en face projection of a registered contrast volume [P][an][sn] restricted to Wc"""
    b0, bn, a0, an, s0, sn = region
    M = int(repeats)
    G = an if G is None else int(G)
    P, Qp = bn // M, an // G
    shifts = np.asarray(shifts).reshape(P, M, Qp)
    out = _fill_bits((P, an), fill)
    ob, ab = out.view(np.uint32), np.ascontiguousarray(angio, dtype=np.float32)
    for p in range(P):
        for a in range(an):
            s = s0 if surface is None else int(surface[p * M, a])
            if s < 0:
                continue
            clo, chi = covered(shifts[p, :, a // G], s0, sn)
            lo, hi = max(s + offset, clo), min(s + offset + thickness - 1, chi)
            if lo > hi:
                continue
            ob[p, a] = np.float32(am.project([ab[p, a, k - s0] for k in range(lo, hi + 1)], function)).view(np.uint32)
    return out
