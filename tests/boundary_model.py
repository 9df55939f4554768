"""Numpy restatement of include/octpipe.h "boundary tracing", written from that comment.  Volumes are float32 [B][A][L]; a region is
(b0, bn, a0, an, s0, sn); a guide and the result are int32 [bn][an] of absolute depth bins, negative = none.

`trace_loops` is the definition in plain loops over A-scans, nodes and candidates on numpy float32 scalars.  `trace` walks the A-scans
and the candidates in the same plain loops and the same order but handles all nodes of a column at once with elementwise float32
operations (each node still does its own adds in the order the definition fixes; nothing is summed across nodes), which keeps the
larger shapes of the GPU tests quick; tests/test_boundary_trace.py holds the two equal bit for bit and checks them against brute-force
enumeration of every path."""
import numpy as np

F = np.float32


def whole(vol):
    B, A, L = vol.shape
    return (0, B, 0, A, 0, L)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _band(region, guide, band):
    s0, sn = region[4], region[5]
    return (s0, s0 + sn - 1) if guide is None else (int(band[0]), int(band[1]))


def penalties(smoothness, max_step):
    """p_j = fl32(lambda * j): one rounded float32 product"""
    return [F(smoothness) * F(j) for j in range(max_step + 1)]


def candidates(max_step):
    """the order in which the candidates are compared"""
    out = [0]
    for i in range(1, max_step + 1):
        out += [-i, i]
    return out


def node_cost(v, d, s0, s1, k, polarity):
    """c of bin d (inside the window) of the A-scan v"""
    def cl(i):
        return min(max(i, s0), s1)
    with np.errstate(all="ignore"):
        up = F(v[cl(d)])
        for i in range(1, k):
            up = F(up + F(v[cl(d + i)]))
        dn = F(v[cl(d - 1)])
        for i in range(2, k + 1):
            dn = F(dn + F(v[cl(d - i)]))
        g = F(up - dn)
    if not np.isfinite(g):
        return F(0.0)
    return F(-g) if polarity > 0 else g


def _walk(E_last, choice, guide_row, lo, s0, s1):
    """(surface row, cost) from the last column's E and the recorded choices"""
    an = len(choice)
    r, best = 0, E_last[0]
    for i in range(1, len(E_last)):
        if E_last[i] < best:
            r, best = i, E_last[i]
    out = np.full(an, -1, np.int32)
    for a in range(an - 1, -1, -1):
        g = 0 if guide_row is None else int(guide_row[a])
        d = g + lo + r
        if g >= 0 and s0 <= d <= s1:
            out[a] = d
        if a > 0:
            r += int(choice[a][r])
    return out, F(best)


def trace_bscan_loops(rows, guide_row, lo, hi, s0, s1, k, polarity, m, smoothness):
    """one B-scan (rows: float32 [an][L]) in plain loops"""
    an, H = len(rows), hi - lo + 1
    p, order = penalties(smoothness, m), candidates(m)
    choice = [[0] * H for _ in range(an)]
    E = None
    for a in range(an):
        g = 0 if guide_row is None else int(guide_row[a])
        cur = []
        for r in range(H):
            d = g + lo + r
            c = node_cost(rows[a], d, s0, s1, k, polarity) if g >= 0 and s0 <= d <= s1 else F(0.0)
            if a == 0:
                cur.append(c)
                continue
            with np.errstate(all="ignore"):
                best, bj = None, 0
                for j in order:
                    if not 0 <= r + j < H:
                        continue
                    t = F(E[r + j] + p[abs(j)])
                    if best is None or t < best:  # j = 0 comes first and is always inside the band
                        best, bj = t, j
                cur.append(F(best + c))
            choice[a][r] = bj
        E = cur
    return _walk(E, choice, guide_row, lo, s0, s1)


def trace_bscan(rows, guide_row, lo, hi, s0, s1, k, polarity, m, smoothness):
    """one B-scan, the nodes of a column at once"""
    an, H = len(rows), hi - lo + 1
    p, order = penalties(smoothness, m), candidates(m)
    r = np.arange(H)
    choice = np.zeros((an, H), np.int8)
    E = None
    with np.errstate(all="ignore"):
        for a in range(an):
            v = np.asarray(rows[a], np.float32)
            g = 0 if guide_row is None else int(guide_row[a])
            d = g + lo + r
            c = np.zeros(H, np.float32)
            if g >= 0:
                def val(i):
                    return v[np.clip(d + i, s0, s1)]
                up = val(0)
                for i in range(1, k):
                    up = up + val(i)
                dn = val(-1)
                for i in range(2, k + 1):
                    dn = dn + val(-i)
                gr = up - dn
                cc = np.where(np.isfinite(gr), -gr if polarity > 0 else gr, F(0.0)).astype(np.float32)
                c = np.where((d >= s0) & (d <= s1), cc, F(0.0)).astype(np.float32)
            if a == 0:
                E = c
                continue
            best = E + p[0]
            bj = np.zeros(H, np.int8)
            for j in order[1:]:
                ok = (r + j >= 0) & (r + j < H)
                t = E[np.clip(r + j, 0, H - 1)] + p[abs(j)]
                take = ok & (t < best)
                best = np.where(take, t, best)
                bj = np.where(take, np.int8(j), bj)
            choice[a] = bj
            E = (best + c).astype(np.float32)
    return _walk(E, choice, guide_row, lo, s0, s1)


def trace(vol, region, guide=None, band=(-16, 16), half_width=2, polarity=1, max_step=1, smoothness=0.0, loops=False):
    """(surface int32 [bn][an], path costs float32 [bn])"""
    b0, bn, a0, an, s0, sn = region
    s1 = s0 + sn - 1
    lo, hi = _band(region, guide, band)
    surface = np.empty((bn, an), np.int32)
    cost = np.empty(bn, np.float32)
    f = trace_bscan_loops if loops else trace_bscan
    for b in range(bn):
        rows = vol[b0 + b, a0:a0 + an]
        surface[b], cost[b] = f(rows, None if guide is None else guide[b], lo, hi, s0, s1, half_width, polarity, max_step, smoothness)
    return surface, cost


def brute_force(rows, guide_row, lo, hi, s0, s1, k, polarity, m, smoothness):
    """every path of one tiny B-scan: (surface row, cost) of the path the definition's tie rules pick.  The cost of a path is summed
    in the recurrence's order, E = (E + p) + c; among equal costs the definition prefers, from the last A-scan backwards, the smallest
    end node and then the candidate order j = 0, -1, +1, ..."""
    import itertools
    an, H = len(rows), hi - lo + 1
    p, order = penalties(smoothness, m), candidates(m)

    def c(a, r):
        g = 0 if guide_row is None else int(guide_row[a])
        d = g + lo + r
        return node_cost(rows[a], d, s0, s1, k, polarity) if g >= 0 and s0 <= d <= s1 else F(0.0)

    best = None
    for path in itertools.product(range(H), repeat=an):
        if any(abs(path[a] - path[a - 1]) > m for a in range(1, an)):
            continue
        e = c(0, path[0])
        for a in range(1, an):
            e = F(F(e + p[abs(path[a] - path[a - 1])]) + c(a, path[a]))
        # the preference among equal costs, read backwards from the last A-scan
        key = [path[-1]] + [order.index(path[a - 1] - path[a]) for a in range(an - 1, 0, -1)]
        if best is None or e < best[0] or (e == best[0] and key < best[1]):
            best = (e, key, path)
    out = np.full(an, -1, np.int32)
    for a in range(an):
        g = 0 if guide_row is None else int(guide_row[a])
        d = g + lo + best[2][a]
        if g >= 0 and s0 <= d <= s1:
            out[a] = d
    return out, best[0]
