"""numpy model of the volume rendering definition (include/octpipe.h "volume rendering"), written from that comment: vectorised over the
pixels, runnable in float64 and in float32 (`dtype`).  Besides the image it reports, per pixel, how close the closest decision of its
march came to flipping -- the pixel's *margin* (intensity units: threshold compares, the running-maximum compare where the mode's colour
depends on which sample wins, the termination tests 0.99 / 0.9, the isosurface hit and its refinement), `kmargin` (how far L / stepLength
is from the integer at which the trip count K changes) and `tmargin` (t_1 - t_0 of the slab test).  A pixel whose margin is small may
legitimately come out different in another arithmetic; the tests excuse such pixels, up to a cap."""
import math

import numpy as np

MIP, DMIP, XRAY, ALPHA_BLENDING, MIDA, ISOSURFACE = 0, 1, 2, 3, 4, 5
MODE_NAMES = {MIP: "MIP", DMIP: "DMIP", XRAY: "XRAY", ALPHA_BLENDING: "ALPHA_BLENDING", MIDA: "MIDA", ISOSURFACE: "ISOSURFACE"}
RGBA_F32, RGBA_U8 = 0, 1
MAX_STEPS = 1733
SLACK = 1e-3  # a compare that is this far from mattering is not a decision of the pixel


def default_settings():
    """the reference's start-up state (the header's octpipe_default_render_settings comment)"""
    return dict(mode=MIP, width=512, height=512, viewMatrix=view_matrix((1, 0, 0, 0), 0.0, 0.0, -500.0), fovDegrees=50.0,
                stretch=(1.0, 1.0, 1.0), stepLength=0.01, threshold=0.5, depthWeight=0.7, alphaExponent=2.0, gamma=2.2, smoothFactor=1,
                shadingEnabled=1, lutEnabled=0, background=(0.0, 0.0, 0.0), material=(1.0, 1.0, 1.0), lightPosition=(1.0, 3.0, 3.0),
                jitterSeed=0, outputFormat=RGBA_F32)


def view_matrix(q, view_x, view_y, dist_exp):
    """translate(viewX, viewY, -4 exp(distExp / 600)) times the rotation of the normalised quaternion (w, x, y, z); float32, row-major"""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q / math.sqrt(float(np.dot(q, q)))
    m = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), view_x],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x), view_y],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y), -4.0 * math.exp(dist_exp / 600.0)],
                  [0, 0, 0, 1]], dtype=np.float64)
    return m.astype(np.float32)


def jitter(px, py, seed):
    """j of step 2 per pixel (float64 array of u8 / 255 numerators, i.e. the byte)"""
    with np.errstate(over="ignore"):
        h = (px.astype(np.uint32) * np.uint32(0x9E3779B1) + py.astype(np.uint32) * np.uint32(0x85EBCA77)
             + np.uint32(seed) * np.uint32(0xC2B2AE3D))
        h ^= h >> np.uint32(15)
        h = h * np.uint32(0x2C1B3C6D)
        h ^= h >> np.uint32(12)
        h = h * np.uint32(0x297A2D39)
        h ^= h >> np.uint32(15)
    return (h >> np.uint32(24)).astype(np.uint32)


def _axis(p, n, dt):
    u = p * dt(n) - dt(0.5)
    u = np.fmin(np.fmax(u, dt(-1.0)), dt(n))
    fl = np.floor(u)
    w = u - fl
    i = fl.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), w


def fetch(vox, p, dt):
    """I(p) of step 3; vox [z][y][x] uint8, p = (x, y, z) arrays of texture coordinates"""
    nz, ny, nx = vox.shape
    x0, x1, wx = _axis(p[0], nx, dt)
    y0, y1, wy = _axis(p[1], ny, dt)
    z0, z1, wz = _axis(p[2], nz, dt)
    v = lambda z, y, x: vox[z, y, x].astype(dt)
    b00 = v(z0, y0, x0) + wx * (v(z0, y0, x1) - v(z0, y0, x0))
    b01 = v(z0, y1, x0) + wx * (v(z0, y1, x1) - v(z0, y1, x0))
    b10 = v(z1, y0, x0) + wx * (v(z1, y0, x1) - v(z1, y0, x0))
    b11 = v(z1, y1, x0) + wx * (v(z1, y1, x1) - v(z1, y1, x0))
    c0 = b00 + wy * (b01 - b00)
    c1 = b10 + wy * (b11 - b10)
    return (c0 + wz * (c1 - c0)) / dt(255.0)


def lut_fetch(lut, i, dt):
    """the colour table at intensity i: (r, g, b) arrays"""
    i0, i1, w = _axis(i, lut.shape[0], dt)
    out = []
    for c in range(3):
        a, b = lut[i0, c].astype(dt), lut[i1, c].astype(dt)
        out.append((a + w * (b - a)) / dt(255.0))
    return out


def _pow(x, y, dt):
    x = np.asarray(x, dtype=dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.exp2(dt(y) * np.log2(np.where(x > 0, x, dt(1.0)))) if np.isscalar(y) else np.exp2(y * np.log2(np.where(x > 0, x, dt(1.0))))
    return np.where(x > 0, r, dt(0.0)).astype(dt)


def _normalize(v, dt):
    l = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    ok = l > 0
    ls = np.where(ok, l, dt(1.0))
    return [np.where(ok, c / ls, dt(0.0)) for c in v]


def normal(vox, p, h, dt):
    e = dt(0.577350269)
    eh = e * dt(h)
    signs = ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))
    n = [np.zeros_like(p[0]), np.zeros_like(p[0]), np.zeros_like(p[0])]
    for s in signs:
        i = fetch(vox, [p[c] + dt(s[c]) * eh for c in range(3)], dt)
        for c in range(3):
            n[c] = n[c] + (dt(s[c]) * e) * i
    u = _normalize(n, dt)
    return [-c for c in u]


def shade(colour, p, ray, N, light, Ia, kd, ks, dt):
    Lv = _normalize([dt(light[c]) - p[c] for c in range(3)], dt)
    nr = _normalize(ray, dt)
    Vw = [-c for c in nr]
    H = _normalize([Lv[c] + Vw[c] for c in range(3)], dt)
    dotp = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    d = dt(Ia) + dt(kd) * np.fmax(dt(0.0), dotp(N, Lv))
    s = dt(ks) * _pow(np.fmax(dt(0.0), dotp(N, H)), 600.0, dt)
    return [d * colour[c] + s for c in range(3)]


def camera(st, dims, dt):
    """the host side of step 1: focal length, aspect, ray origin, box top -- as the library computes them (double, rounded to float32;
    the box in float32), then cast to the working precision"""
    V = np.asarray(st["viewMatrix"], dtype=np.float32).reshape(4, 4)
    R = V[:3, :3].astype(np.float64)
    t = V[:3, 3].astype(np.float64)
    origin = (-np.linalg.solve(R, t)).astype(np.float32)
    focal = np.float32(1.0 / math.tan(float(np.float32(st["fovDegrees"])) * math.pi / 180.0 / 2.0))
    aspect = np.float32(float(st["width"]) / float(st["height"]))
    e = np.asarray(dims, dtype=np.float32) * np.asarray(st["stretch"], dtype=np.float32)
    top = (e / e.max()) / np.float32(2.0)
    return V[:3, :3].astype(dt), origin.astype(dt), dt(focal), dt(aspect), top.astype(dt)


def box_top(dims, stretch):
    e = np.asarray(dims, dtype=np.float32) * np.asarray(stretch, dtype=np.float32)
    return (e / e.max()) / np.float32(2.0)


def render(vox, settings, lut=None, dtype=np.float64):
    """Render vox ([z][y][x] uint8) with `settings` (a dict with the fields of OctPipeRenderSettings).  Returns a dict: image
    [height][width][4] (dtype; uint8 for RGBA_U8), hit [height][width] (t_1 > t_0), margin, kmargin, tmargin [height][width] (inf where
    no decision was taken), samples (total number of voxel fetches of the march, without the normals)."""
    dt = np.dtype(dtype).type
    st = settings
    vox = np.ascontiguousarray(vox, dtype=np.uint8)
    nz, ny, nx = vox.shape
    W, H, mode = int(st["width"]), int(st["height"]), int(st["mode"])
    R, o, focal, aspect, top = camera(st, (nx, ny, nz), dt)
    step, thr = dt(np.float32(st["stepLength"])), dt(np.float32(st["threshold"]))
    dw, aexp = dt(np.float32(st["depthWeight"])), dt(np.float32(st["alphaExponent"]))
    gamma = float(np.float32(st["gamma"]))
    inv_gamma = dt(np.float32(1.0 / gamma))
    bg = [dt(np.float32(c)) for c in st["background"]]
    bg_gamma = [dt(np.float32(float(np.float32(c)) ** gamma if c > 0 else 0.0)) for c in st["background"]]
    light = [np.float32(c) for c in st["lightPosition"]]
    material = [dt(np.float32(c)) for c in st["material"]]
    use_lut = bool(st["lutEnabled"]) and mode != ISOSURFACE
    if use_lut:
        lut = np.ascontiguousarray(lut, dtype=np.uint8)
    shading = bool(st["shadingEnabled"])

    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px, py = px.ravel(), py.ravel()
    n = px.size
    # step 1
    cx = (dt(2.0) * (px.astype(dt) + dt(0.5)) / dt(W) - dt(1.0)) * aspect
    cy = dt(2.0) * (py.astype(dt) + dt(0.5)) / dt(H) - dt(1.0)
    cz = np.full(n, -focal, dtype=dt)
    d = [cx * R[0, j] + cy * R[1, j] + cz * R[2, j] for j in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lo, hi = [], []
        for i in range(3):
            inv = dt(1.0) / d[i]
            a, b = inv * (top[i] - o[i]), inv * (-top[i] - o[i])
            lo.append(np.fmin(a, b))
            hi.append(np.fmax(a, b))
        t0 = np.fmax(dt(0.0), np.fmax(np.fmax(lo[0], lo[1]), lo[2]))
        t1 = np.fmin(np.fmin(hi[0], hi[1]), hi[2])
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
        K = np.where(kf > 0, np.fmin(kf, dt(MAX_STEPS)), dt(0.0))
        K = np.where(np.isnan(K), 0, K).astype(np.int64)
    K = np.where(hit, K, 0)
    kmargin = np.where(hit, np.abs(x - np.rint(x)), np.inf).astype(np.float64)
    if int(st["jitterSeed"]):
        j = jitter(px, py, int(st["jitterSeed"])).astype(dt) / dt(255.0)
        start = [start[i] + sv[i] * j for i in range(3)]

    margin = np.full(n, np.inf)
    m = np.zeros(n, dt)
    total = np.zeros(n, dt)
    count = np.zeros(n, np.int64)
    C = [np.zeros(n, dt) for _ in range(3)]
    Ca = np.zeros(n, dt)
    pmax = [s.copy() for s in start]
    hitpos = [s.copy() for s in start]
    found = np.zeros(n, bool)
    done = np.zeros(n, bool)
    samples = 0

    def note(mask, value):
        if mask.any():
            margin[mask] = np.minimum(margin[mask], np.abs(value[mask]).astype(np.float64))

    def transfer_rgb(i):
        if use_lut:
            return lut_fetch(lut, i, dt)
        if mode == DMIP:
            return [i + (dt(1.0) - i) * dt(0.1), i, i + (dt(1.0) - i) * dt(0.2)]
        return [i, i, i]

    for k in range(int(K.max()) if n else 0):
        act = (k < K) & ~done
        if not act.any():
            break
        samples += int(act.sum())
        p = [start[i] + sv[i] * dt(k) for i in range(3)]
        I = fetch(vox, p, dt)
        if mode in (MIP, DMIP):
            note(act & (I > m - dt(SLACK)), I - thr)
            if mode == DMIP:
                note(act & (I > thr - dt(SLACK)), I - m)
            upd = act & (I > m) & (I > thr)
            m = np.where(upd, I, m)
            if mode == DMIP:
                pmax = [np.where(upd, p[i], pmax[i]) for i in range(3)]
            note(act, m - dt(0.99))
            done |= act & ~(m < dt(0.99))
        elif mode == XRAY:
            note(act, I - thr)
            upd = act & (I > thr)
            total = np.where(upd, total + I, total)
            count += upd
        elif mode == ALPHA_BLENDING:
            note(act, I - thr)
            upd = act & (I > thr)
            c = transfer_rgb(I)
            ca = _pow(I, aexp, dt)
            q = (dt(1.0) - ca) * Ca
            nC = [ca * c[i] + q * C[i] for i in range(3)]
            nCa = ca + (dt(1.0) - ca) * Ca
            cue = _pow(np.full(n, 2.25, dt), (L - dt(k) * step) / Ls, dt) / dt(1.75)
            nC = [nCa * nC[i] * cue for i in range(3)]
            if shading and upd.any():
                nC = shade(nC, p, ray, normal(vox, p, 0.005, dt), light, 0.75, 0.5, 1.0, dt)
            C = [np.where(upd, nC[i], C[i]) for i in range(3)]
            Ca = np.where(upd, nCa, Ca)
            note(act, Ca - dt(0.9))
            done |= act & ~(Ca < dt(0.9))
        elif mode == MIDA:
            note(act & (I > m - dt(SLACK)), I - thr)
            note(act & (I > thr - dt(SLACK)), I - m)
            upd = act & (I > thr) & (I > m)
            c = transfer_rgb(I)
            ca = _pow(I, aexp, dt)
            w = dt(1.0) - (I - m)
            q = (dt(1.0) - w * Ca) * ca
            nC = [w * C[i] + q * c[i] for i in range(3)]
            nCa = w * Ca + q
            if shading and upd.any():
                nC = shade(nC, p, ray, normal(vox, p, 0.005, dt), light, 0.75, 0.35, 0.2, dt)
            C = [np.where(upd, nC[i], C[i]) for i in range(3)]
            Ca = np.where(upd, nCa, Ca)
            m = np.where(upd, I, m)
            note(act, Ca - dt(0.9))
            done |= act & ~(Ca < dt(0.9))
        else:
            note(act, I - thr)
            upd = act & (I > thr)
            hitpos = [np.where(upd, p[i], hitpos[i]) for i in range(3)]
            found |= upd
            done |= upd

    if mode == ISOSURFACE:
        out = [np.full(n, bg[i], dt) for i in range(3)]
        if found.any():
            q = [hitpos[i] - sv[i] * dt(0.5) for i in range(3)]
            I2 = fetch(vox, q, dt)
            note(found, I2 - thr)
            f = np.where(I2 > thr, dt(0.25), dt(-0.25))
            q = [q[i] - sv[i] * f for i in range(3)]
            ns = int(st["smoothFactor"])
            if ns > 0:
                acc = [np.zeros(n, dt) for _ in range(3)]
                for x_ in range(-ns, ns + 1):
                    for y_ in range(-ns, ns + 1):
                        for z_ in range(-ns, ns + 1):
                            nn = normal(vox, [q[0] + dt(x_) * dt(0.001), q[1] + dt(y_) * dt(0.001), q[2] + dt(z_) * dt(0.001)], 0.001, dt)
                            acc = [acc[i] + nn[i] for i in range(3)]
                cnt = dt((2 * ns + 1) ** 3)
                N = _normalize([acc[i] / cnt for i in range(3)], dt)
            else:
                N = normal(vox, q, 0.001, dt)
            sh = shade(material, q, ray, N, light, 0.2, 0.7, 1.5, dt)
            out = [np.where(found, _pow(sh[i], inv_gamma, dt), out[i]) for i in range(3)]
    else:
        if mode in (MIP, DMIP, XRAY):
            if mode == XRAY:
                m = np.where(count > 0, np.sqrt(total / np.maximum(count, 1).astype(dt)), dt(0.0))
            C = transfer_rgb(m)
            Ca = _pow(m, aexp, dt)
            if mode == DMIP:
                dl = lambda a, b: np.sqrt(sum((a[i] - b[i]) * (a[i] - b[i]) for i in range(3)))
                den = dl(stop, start)
                depth = dl(pmax, start) / np.where(den > 0, den, dt(1.0))
                f = (dt(1.0) - dw) + dt(2.0) * dw * (dt(1.0) - depth)
                C = [C[i] * f for i in range(3)]
                Ca = Ca * f
        out = [_pow(Ca * C[i] + (dt(1.0) - Ca) * bg_gamma[i], inv_gamma, dt) for i in range(3)]

    img = np.empty((n, 4), dt)
    for i in range(3):
        c = np.where(hit, out[i], bg[i])
        img[:, i] = np.fmin(np.fmax(np.where(np.isnan(c), dt(0.0), c), dt(0.0)), dt(1.0))
    img[:, 3] = dt(1.0)
    img = img.reshape(H, W, 4)
    if int(st["outputFormat"]) == RGBA_U8:
        img = quantise(img)
    shape = (H, W)
    return dict(image=img, hit=hit.reshape(shape), margin=margin.reshape(shape), kmargin=kmargin.reshape(shape), tmargin=tmargin.reshape(shape),
                samples=samples)


def quantise(img):
    """RGBA_U8 of step 5 from an RGBA_F32 image, in the image's own precision"""
    dt = img.dtype.type
    return (img * dt(255.0) + dt(0.5)).astype(np.uint8)


def fragile(res, margin_bound, k_bound, t_bound):
    """the pixels excused from the colour comparison"""
    return res["hit"] & ((res["margin"] < margin_bound) | (res["kmargin"] < k_bound) | (res["tmargin"] < t_bound))
