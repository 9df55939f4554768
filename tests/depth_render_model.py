"""numpy model of the OCT Depth render mode and the surface map it is built on (include/octpipe.h "volume rendering", step 4 "OCT_DEPTH"
and "surface map"), written from that comment.  Camera, voxel fetch, colour table, pow, shade and jitter are render_model's; the surface
pre-pass, the depth field, its fetch and the march from the far end are restated here.  Like render_model.render it runs in float64
and in float32 and reports, per pixel, how close the closest decision of the march came to flipping: `margin` is the smallest distance of
any of the four compares of a sample (I > threshold, I < 0.9, D > 0.1, dd < 1.01 stepLength) from its bound, over the samples at which
that compare decides (the other three hold, or miss by less than render_model.SLACK); `kmargin` and `tmargin` are render_model's.
render_model.fragile applies unchanged."""
import numpy as np

import render_model as rm

OCT_DEPTH = 6
MODE_NAME = "OCT Depth"


def depth_threshold(threshold):
    """T of the pre-pass for a render threshold: one float32 product"""
    return np.float32(1.5) * np.float32(threshold)


def surface_start(nz):
    """the highest index the pre-pass examines: (int)(Z - Z / 32.0f) in float32"""
    z = np.float32(nz)
    return int(z - z / np.float32(32.0))


def surface_map(vox, T):
    """s(x, y) as uint16 [y][x]: the largest i in 1 .. start with (float)vox[i][y][x] / 255.0f > T (float32 on both sides), 0 without one"""
    vox = np.ascontiguousarray(vox, dtype=np.uint8)
    nz = vox.shape[0]
    start = min(surface_start(nz), nz - 1)
    hit = vox.astype(np.float32) / np.float32(255.0) > np.float32(T)
    hit[0] = False
    hit[start + 1:] = False
    idx = np.arange(nz, dtype=np.int64)[:, None, None]
    return np.where(hit, idx, 0).max(axis=0).astype(np.uint16)


def depth_texel(s, i, nz, dt):
    """D(x, y, i) for the surface index s of the column: the closed form, in dt"""
    s = s.astype(np.int64)
    d = dt(1.0) - (s - 1 - i).astype(dt) * (dt(1.0) / dt(nz))
    return np.where((i >= 1) & (i < s), d, dt(0.0)).astype(dt)


def depth_fetch(smap, dims, p, dt):
    """Dtex(p): the fetch of step 3 applied to D -- the same indices, weights and blend order as render_model.fetch"""
    nx, ny, nz = dims
    x0, x1, wx = rm._axis(p[0], nx, dt)
    y0, y1, wy = rm._axis(p[1], ny, dt)
    z0, z1, wz = rm._axis(p[2], nz, dt)
    v = lambda z, y, x: depth_texel(smap[y, x], z, nz, dt)
    b00 = v(z0, y0, x0) + wx * (v(z0, y0, x1) - v(z0, y0, x0))
    b01 = v(z0, y1, x0) + wx * (v(z0, y1, x1) - v(z0, y1, x0))
    b10 = v(z1, y0, x0) + wx * (v(z1, y0, x1) - v(z1, y0, x0))
    b11 = v(z1, y1, x0) + wx * (v(z1, y1, x1) - v(z1, y1, x0))
    c0 = b00 + wy * (b01 - b00)
    c1 = b10 + wy * (b11 - b10)
    return c0 + wz * (c1 - c0)


def render(vox, settings, lut=None, dtype=np.float64):
    """Render vox ([z][y][x] uint8) in the OCT Depth mode with `settings` (the fields of OctPipeRenderSettings; `mode` is not looked at).
    Returns what render_model.render returns, plus `surface` (the map the image was rendered with)."""
    dt = np.dtype(dtype).type
    st = settings
    vox = np.ascontiguousarray(vox, dtype=np.uint8)
    nz, ny, nx = vox.shape
    W, H = int(st["width"]), int(st["height"])
    R, o, focal, aspect, top = rm.camera(st, (nx, ny, nz), dt)
    step, thr = dt(np.float32(st["stepLength"])), dt(np.float32(st["threshold"]))
    aexp = dt(np.float32(st["alphaExponent"]))
    gamma = float(np.float32(st["gamma"]))
    inv_gamma = dt(np.float32(1.0 / gamma))
    bg = [dt(np.float32(c)) for c in st["background"]]
    bg_gamma = [dt(np.float32(float(np.float32(c)) ** gamma if c > 0 else 0.0)) for c in st["background"]]
    light = [np.float32(c) for c in st["lightPosition"]]
    use_lut = bool(st["lutEnabled"])
    if use_lut:
        lut = np.ascontiguousarray(lut, dtype=np.uint8)
    shading = bool(st["shadingEnabled"])
    smap = surface_map(vox, depth_threshold(st["threshold"]))
    # the compares' constants as the float32 kernel holds them
    hi, dmin, dd_max, lut_shift = dt(np.float32(0.9)), dt(np.float32(0.1)), dt(np.float32(1.01) * np.float32(st["stepLength"])), dt(np.float32(0.05))

    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px, py = px.ravel(), py.ravel()
    n = px.size
    # step 1
    cx = (dt(2.0) * (px.astype(dt) + dt(0.5)) / dt(W) - dt(1.0)) * aspect
    cy = dt(2.0) * (py.astype(dt) + dt(0.5)) / dt(H) - dt(1.0)
    cz = np.full(n, -focal, dtype=dt)
    d = [cx * R[0, j] + cy * R[1, j] + cz * R[2, j] for j in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lo, up = [], []
        for i in range(3):
            inv = dt(1.0) / d[i]
            a, b = inv * (top[i] - o[i]), inv * (-top[i] - o[i])
            lo.append(np.fmin(a, b))
            up.append(np.fmax(a, b))
        t0 = np.fmax(dt(0.0), np.fmax(np.fmax(lo[0], lo[1]), lo[2]))
        t1 = np.fmin(np.fmin(up[0], up[1]), up[2])
        hit = t1 > t0
        tmargin = np.where(hit, t1 - t0, np.inf).astype(np.float64)
        # step 2
        size = [top[i] - (-top[i]) for i in range(3)]
        t0h, t1h = np.where(hit, t0, dt(0.0)), np.where(hit, t1, dt(1.0))
        start = [(o[i] + d[i] * t0h - (-top[i])) / size[i] for i in range(3)]
        stop = [(o[i] + d[i] * t1h - (-top[i])) / size[i] for i in range(3)]
        ray = [stop[i] - start[i] for i in range(3)]
        L = np.sqrt(ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2])
        Ls = np.where(L > 0, L, dt(1.0))
        sv = [step * ray[i] / Ls for i in range(3)]
        x = L / step
        kf = np.ceil(x)
        K = np.where(kf > 0, np.fmin(kf, dt(rm.MAX_STEPS)), dt(0.0))
        K = np.where(np.isnan(K), 0, K).astype(np.int64)
    K = np.where(hit, K, 0)
    kmargin = np.where(hit, np.abs(x - np.rint(x)), np.inf).astype(np.float64)
    far = stop
    if int(st["jitterSeed"]):
        j = rm.jitter(px, py, int(st["jitterSeed"])).astype(dt) / dt(255.0)
        far = [stop[i] + sv[i] * j for i in range(3)]

    margin = np.full(n, np.inf)
    C = [np.zeros(n, dt) for _ in range(3)]
    Ca = np.zeros(n, dt)
    Dold = np.ones(n, dt)
    samples = 0
    slack = dt(rm.SLACK)
    for k in range(int(K.max()) if n else 0):
        act = k < K
        if not act.any():
            break
        samples += int(act.sum())
        q = [far[i] - sv[i] * dt(k) for i in range(3)]
        I = rm.fetch(vox, q, dt)
        D = depth_fetch(smap, (nx, ny, nz), q, dt)
        dd = np.abs(D - Dold)
        Dold = np.where(act, D, Dold)
        # signed distances of the four compares from their bounds: positive holds
        dist = [I - thr, hi - I, D - dmin, dd_max - dd]
        for c in range(4):
            others = act
            for e in range(4):
                if e != c:
                    others = others & (dist[e] > -slack)
            if others.any():
                margin[others] = np.minimum(margin[others], np.abs(dist[c][others]).astype(np.float64))
        upd = act & (I > thr) & (I < hi) & (D > dmin) & (dd < dd_max)
        if not upd.any():
            continue
        if use_lut:
            c = rm.lut_fetch(lut, D - lut_shift, dt)
            ca = rm._pow(I, aexp, dt)
        else:
            c = [D, D, D]
            ca = rm._pow(D, aexp, dt)
        q_ = (dt(1.0) - ca) * Ca
        nC = [ca * c[i] + q_ * C[i] for i in range(3)]
        nCa = ca + q_
        nCs = np.where(upd, nCa, dt(1.0))
        nC = [nC[i] / nCs for i in range(3)]
        if shading:
            nC = rm.shade(nC, q, ray, rm.normal(vox, q, 0.005, dt), light, 0.75, 0.5, 1.0, dt)
        C = [np.where(upd, nC[i], C[i]) for i in range(3)]
        Ca = np.where(upd, nCa, Ca)

    out = [rm._pow(Ca * C[i] + (dt(1.0) - Ca) * bg_gamma[i], inv_gamma, dt) for i in range(3)]
    img = np.empty((n, 4), dt)
    for i in range(3):
        c = np.where(hit, out[i], bg[i])
        img[:, i] = np.fmin(np.fmax(np.where(np.isnan(c), dt(0.0), c), dt(0.0)), dt(1.0))
    img[:, 3] = dt(1.0)
    img = img.reshape(H, W, 4)
    if int(st["outputFormat"]) == rm.RGBA_U8:
        img = rm.quantise(img)
    shape = (H, W)
    return dict(image=img, hit=hit.reshape(shape), margin=margin.reshape(shape), kmargin=kmargin.reshape(shape), tmargin=tmargin.reshape(shape),
                samples=samples, surface=smap)
