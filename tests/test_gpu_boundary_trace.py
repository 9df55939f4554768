"""Boundary tracing on the MI355X (include/octpipe.h "boundary tracing", csrc/boundary_trace.h, csrc/pipe_boundary.hip).

Every result is compared bit for bit against the numpy model of tests/boundary_model.py: surfaces as int32, path costs as uint32.  There
is no tolerance and nothing is excused.  Small shapes through data= on small handles; every case runs the public call and every `form`
of the kernel that applies to it (one wave or one workgroup per B-scan, the choices in LDS or in scratch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import boundary_model as bm
import surface_model as sm
from octproz_amd import OctPipeError, Pipeline, synthetic_raw, v180_benchmark_params

pytestmark = pytest.mark.gpu

# the kernel's geometry (csrc/boundary_trace.h): the wave form's nodes, and the bytes of 4-bit choices each form keeps in LDS
WAVE_H, CH_WAVE, CH_WG = 64, 32768, 147328
ERR_INVALID_ARGUMENT = 1


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(g, w):
        i = np.argwhere(g != w)
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %s (%#x), want %s (%#x)" % (
            what, len(i), g.size, tuple(i[0]), got[tuple(i[0])], g[tuple(i[0])], want[tuple(i[0])], w[tuple(i[0])]))


def _fetch(ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def _dev(raw):
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.int16)).to("cuda:0")


def _kw(region):
    b0, bn, a0, an, s0, sn = region
    return dict(bscans=(b0, bn), ascans=(a0, an), depth=(s0, sn))


def _forms(region, guide, band):
    """the form codes that apply (include/octpipe_debug.h), and the one the public call picks"""
    H = region[5] if guide is None else band[1] - band[0] + 1
    choices = region[3] * ((H + 1) // 2)
    ok = [4] + ([3] if choices <= CH_WG else [])
    if H <= WAVE_H:
        ok += [2] + ([1] if choices <= CH_WAVE else [])
    pick = (1 if choices <= CH_WAVE else 2) if H <= WAVE_H else (3 if choices <= CH_WG else 4)
    return sorted(ok), pick


def _check(pipe, vol, region, what, guide=None, band=(-16, 16), **settings):
    """the public call and every form that applies against the model; returns the model's result"""
    want_s, want_c = bm.trace(vol, region, guide=guide, band=band, **settings)
    kw = dict(guide=guide, band=band, cost=True, data=vol, **settings, **_kw(region))
    s, c = pipe.trace_boundary(**kw)
    _same(s, want_s, (what, "surface"))
    _same(c, want_c, (what, "cost"))
    _same(pipe.trace_boundary(**dict(kw, cost=False)), want_s, (what, "surface without costs"))
    forms, pick = _forms(region, guide, band)
    for form in forms:
        (s, c), ms = pipe.trace_boundary_timed(form=form, **kw)
        _same(s, want_s, (what, "form", form, "surface"))
        _same(c, want_c, (what, "form", form, "cost"))
        assert ms > 0.0
    for form in set((1, 2, 3, 4)) - set(forms):
        with pytest.raises(OctPipeError) as e:
            pipe.trace_boundary_timed(form=form, **kw)
        assert e.value.code == ERR_INVALID_ARGUMENT and "form" in str(e.value), (what, form)
    return want_s, want_c


SETTINGS = [dict(half_width=2, polarity=1, max_step=1, smoothness=0.0), dict(half_width=8, polarity=-1, max_step=7, smoothness=0.37),
            dict(half_width=1, polarity="rising", max_step=2, smoothness=0.37), dict(half_width=3, polarity="falling", max_step=7, smoothness=0.0)]
_POL = {"rising": 1, "falling": -1}


def _model_settings(s):
    return dict(s, polarity=_POL.get(s["polarity"], s["polarity"]))


def _check_named(pipe, vol, region, what, settings, **kw):
    """_check with a polarity given by name: the model takes the number"""
    want = bm.trace(vol, region, guide=kw.get("guide"), band=kw.get("band", (-16, 16)), **_model_settings(settings))
    got = pipe.trace_boundary(cost=True, data=vol, **settings, **kw, **_kw(region))
    _same(got[0], want[0], (what, "named polarity"))
    _same(got[1], want[1], (what, "named polarity, cost"))


@pytest.fixture(scope="module")
def small():
    """N = 256 (depth 128), 67 A-scans, 5 B-scans"""
    pipe = Pipeline(v180_benchmark_params(256, 67, 5), device=0)
    vol = np.random.default_rng(11).standard_normal((5, 67, 128)).astype(np.float32)
    yield pipe, vol
    pipe.close()


@pytest.fixture(scope="module")
def deep():
    """N = 2048 (depth 1024), 9 A-scans, 2 B-scans"""
    pipe = Pipeline(v180_benchmark_params(2048, 9, 2), device=0)
    vol = np.random.default_rng(12).standard_normal((2, 9, 1024)).astype(np.float32)
    yield pipe, vol
    pipe.close()


@pytest.fixture(scope="module")
def many():
    """N = 256 (depth 128), 2400 A-scans, one B-scan: enough A-scans to push the choices of either form out of LDS"""
    pipe = Pipeline(v180_benchmark_params(256, 2400, 1), device=0)
    vol = np.random.default_rng(13).standard_normal((1, 2400, 128)).astype(np.float32)
    yield pipe, vol
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("H", [1, 2, 63, 64, 65, 128])
def test_unguided_node_and_ascan_counts(small, H):
    """H at the border between the wave and the workgroup form and at the workgroup-size border; 1, 2, 3 and 65 A-scans; m = 7 with
    H < m; a region with firstBscan, firstAscan and firstSample > 0; one and five B-scans"""
    pipe, vol = small
    first = 128 - H if H > 100 else 5
    for i, an in enumerate((1, 2, 3, 65)):
        for n, s in enumerate(SETTINGS):
            region = (0, 5, 2, an, first, H) if (an, n) == (3, 1) else (1 + i, 1, min(i, 67 - an), an, first, H)
            if isinstance(s["polarity"], str):
                _check_named(pipe, vol, region, ("unguided", H, an, n), s)
            else:
                _check(pipe, vol, region, ("unguided", H, an, n), **s)


@pytest.mark.parametrize("an", [1, 9])
def test_unguided_1024_nodes(deep, an):
    pipe, vol = deep
    _check(pipe, vol, (0, 2, 0, an, 0, 1024), ("H = 1024", an), half_width=2, max_step=1, smoothness=0.37)
    _check(pipe, vol, (1, 1, 9 - an, an, 0, 1024), ("H = 1024, m = 7", an), half_width=8, polarity=-1, max_step=7, smoothness=0.0)


def test_clamped_gradient_on_a_three_bin_window(small):
    pipe, vol = small
    for s0 in (0, 60, 125):
        _check(pipe, vol, (0, 5, 0, 67, s0, 3), ("k = 8 on 3 bins", s0), half_width=8, max_step=7, smoothness=0.37)
        _check(pipe, vol, (2, 1, 1, 65, s0, 3), ("k = 8 on 3 bins, falling", s0), half_width=8, polarity=-1, max_step=1, smoothness=0.0)


def test_choices_pushed_from_lds_into_scratch(many):
    """2400 A-scans: 64 nodes need 76 800 bytes of choices (the wave form keeps 32 768 in LDS), 128 nodes 153 600 (the workgroup form keeps
    147 328); the public call takes the scratch form and _check sees the LDS form of the kind refused; 2301 A-scans of 128 nodes still fit"""
    pipe, vol = many
    assert _forms((0, 1, 0, 2400, 30, 64), None, None) == ([2, 3, 4], 2) and _forms((0, 1, 0, 2400, 0, 128), None, None) == ([4], 4)
    assert _forms((0, 1, 0, 2301, 0, 128), None, None) == ([3, 4], 3) and _forms((0, 1, 0, 2302, 0, 128), None, None) == ([3, 4], 3)
    assert _forms((0, 1, 0, 2303, 0, 128), None, None) == ([4], 4)
    _check(pipe, vol, (0, 1, 0, 2400, 30, 64), "wave form, scratch", half_width=2, max_step=2, smoothness=0.37)
    _check(pipe, vol, (0, 1, 0, 2400, 0, 128), "workgroup form, scratch", half_width=2, max_step=2, smoothness=0.37)
    _check(pipe, vol, (0, 1, 50, 2302, 0, 128), "workgroup form, the last size in LDS", half_width=1, max_step=7, smoothness=0.0)
    _check(pipe, vol, (0, 1, 50, 2303, 0, 128), "workgroup form, the first size in scratch", half_width=1, max_step=7, smoothness=0.0)
    guide = np.full((1, 1025), 60, np.int32)
    _check(pipe, vol, (0, 1, 3, 1024, 0, 128), "wave form, the last size in LDS", guide=guide[:, :1024], band=(-32, 31), max_step=3, smoothness=0.37)
    _check(pipe, vol, (0, 1, 3, 1025, 0, 128), "wave form, the first size in scratch", guide=guide, band=(-32, 31), max_step=3, smoothness=0.37)


# ---------------------------------------------------------------------------------------------------------------------- 2. values
@pytest.mark.parametrize("kind", ["three-values", "constant", "non-finite", "huge"])
def test_ties_and_non_finite_values(small, kind):
    pipe, _ = small
    rng = np.random.default_rng(len(kind))
    if kind == "three-values":  # almost every compare ties: the order of the candidates decides
        vol = rng.integers(0, 3, (5, 67, 128)).astype(np.float32)
    elif kind == "constant":
        vol = np.full((5, 67, 128), 1.5, np.float32)
    elif kind == "huge":  # sums overflow to +-inf, E follows IEEE
        with np.errstate(over="ignore"):  # (some values become +-inf)
            vol = (rng.standard_normal((5, 67, 128)) * 2e38).astype(np.float32)
    else:
        vol = rng.standard_normal((5, 67, 128)).astype(np.float32)
        flat = vol.reshape(-1)
        where = rng.choice(flat.size, flat.size // 30, replace=False)
        flat[where[0::3]], flat[where[1::3]], flat[where[2::3]] = np.nan, np.inf, -np.inf
    for region in ((0, 5, 0, 67, 0, 128), (0, 2, 1, 65, 20, 40), (4, 1, 0, 67, 3, 65)):
        for s in SETTINGS[:2]:
            _check(pipe, vol, region, (kind, region), **s)
        _check(pipe, vol, region, (kind, region, "lambda = 1"), half_width=2, max_step=2, smoothness=1.0)


def test_path_cost_bits(small):
    pipe, vol = small
    const = np.full((5, 67, 128), 2.0, np.float32)
    # one A-scan of a constant volume: g = +0, c = -0 for polarity +1, and E = c with its own bits
    _, c = _check(pipe, const, (0, 5, 7, 1, 10, 30), "-0", half_width=2, polarity=1)
    assert c.view(np.uint32).tolist() == [0x80000000] * 5
    _, c = _check(pipe, const, (0, 5, 7, 1, 10, 30), "+0", half_width=2, polarity=-1)
    assert c.view(np.uint32).tolist() == [0] * 5
    _, c = _check(pipe, const, (0, 5, 7, 2, 10, 30), "(-0 + +0) + -0", half_width=2, polarity=1)
    assert c.view(np.uint32).tolist() == [0] * 5
    guide = np.full((5, 1), 20, np.int32)
    _, c = _check(pipe, const, (0, 5, 7, 1, 10, 30), "-0, guided", guide=guide, band=(-3, 3), half_width=8)
    assert c.view(np.uint32).tolist() == [0x80000000] * 5
    s, c = _check(pipe, vol, (0, 5, 0, 67, 0, 128), "costs of five B-scans", half_width=2, max_step=2, smoothness=0.37)
    assert len(set(c.view(np.uint32).tolist())) == 5 and (s >= 0).all()


# ---------------------------------------------------------------------------------------------------------------------- 3. guides
@pytest.mark.parametrize("band", [(-16, 16), (-40, 40), (0, 0), (3, 66), (-70, -6)], ids=lambda b: "band%d_%d" % b)
def test_guides(small, band):
    pipe, vol = small
    rng = np.random.default_rng(band[1] - band[0])
    region = (0, 5, 1, 65, 8, 112)  # W = [8, 119]
    smooth = (60 + 10 * np.sin(np.arange(65) / 9.0)[None, :] + np.arange(5)[:, None]).astype(np.int32)
    holes = smooth.copy()
    holes[rng.random(holes.shape) < 0.3] = -1 - rng.integers(0, 5)
    holes[2, :] = -2  # a B-scan without a guide
    jumps = rng.integers(8, 120, (5, 65)).astype(np.int32)  # neighbouring entries differ by more than m
    partly = np.linspace(-30, 160, 65).astype(np.int32)[None, :].repeat(5, 0)  # the band leaves W at either end (negative: no guide)
    outside = np.full((5, 65), 400, np.int32)  # the whole band outside W
    edge = np.full((5, 65), 2 ** 31 - 1, np.int32)
    for name, guide in (("smooth", smooth), ("holes", holes), ("jumps", jumps), ("partly outside", partly), ("outside", outside), ("int max", edge)):
        for s in SETTINGS[:2]:
            want, _ = _check(pipe, vol, region, (name, band), guide=guide, band=band, **s)
        if name == "outside" or name == "int max":
            assert (want == -1).all()
    _check_named(pipe, vol, region, ("named", band), SETTINGS[2], guide=holes, band=band)
    _check(pipe, vol, (3, 1, 0, 1, 0, 128), ("one A-scan", band), guide=np.array([[64]], np.int32), band=band, half_width=4)


# ---------------------------------------------------------------------------------------------------------------------- 4. sources, results
def test_sources_results_and_repeats():
    n, a, b = 1024, 96, 2
    pipe = Pipeline(v180_benchmark_params(n, a, b, buffers_per_volume=2), device=0)
    for i in range(2):
        pipe.octCudaPipeline(synthetic_raw(n, a, b, seed=170 + i))
        pipe.synchronize()
    _, _, last = pipe.processed_device()
    region = (0, 2, 5, 80, 9, 400)
    kw = dict(cost=True, half_width=2, max_step=2, smoothness=0.37, **_kw(region))
    per_slot = []
    for slot in (0, 1):
        host = pipe.processed_host(slot=slot).reshape(b, a, n // 2).copy()
        dvol = torch.from_numpy(host).cuda()
        want = bm.trace(host, region, half_width=2, max_step=2, smoothness=0.37)
        guide = np.clip(want[0] - 9, 0, None).astype(np.int32)
        want_g = bm.trace(host, region, guide=guide, band=(-20, 20), half_width=2, max_step=2, smoothness=0.37)
        dguide = torch.from_numpy(guide).cuda()
        for what, src in (("the handle's volume", dict(buffer=slot)), ("repeat", dict(buffer=slot)), ("host source", dict(data=host)),
                          ("device source", dict(data=dvol))):
            s, c = pipe.trace_boundary(**src, **kw)
            _same(s, want[0], (what, slot))
            _same(c, want[1], (what, slot, "cost"))
            for g in (guide, dguide):
                s, c = pipe.trace_boundary(guide=g, band=(-20, 20), **src, **kw)
                _same(s, want_g[0], (what, slot, "guided"))
                _same(c, want_g[1], (what, slot, "guided cost"))
            # a device result: the surface and the costs stay on the device, the call returns the tensor it was given
            out = torch.full((2, 80), -77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            s, c = pipe.trace_boundary(guide=dguide, band=(-20, 20), out=out, **src, **kw)
            assert s is out and c.is_cuda
            pipe.synchronize()
            _same(out.cpu().numpy(), want_g[0], (what, slot, "device result"))
            _same(c.cpu().numpy(), want_g[1], (what, slot, "device costs"))
        per_slot.append(want)
    _same(pipe.trace_boundary(**kw)[0], per_slot[last][0], "the slot written last")
    assert not np.array_equal(per_slot[0][0], per_slot[1][0])
    with pytest.raises(OctPipeError):
        pipe.trace_boundary(buffer=2, **kw)
    pipe.close()


def test_a_host_source_staged_in_several_chunks():
    """72 MB of rows in 9 B-scans: a host source travels in two chunks of whole B-scans (64 MiB each at most); the bits are those of the
    device source, and the B-scans on either side of the border are the model's"""
    n, a, b = 4096, 1024, 9
    depth = n // 2
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    vol = np.random.default_rng(14).standard_normal((b, a, depth), dtype=np.float32)
    assert vol.nbytes > (64 << 20) and (64 << 20) // (4 * depth * a) == 8
    kw = dict(cost=True, half_width=2, max_step=1, smoothness=0.37, depth=(1000, 100))
    s, c = pipe.trace_boundary(data=vol, **kw)
    sd, cd = pipe.trace_boundary(data=torch.from_numpy(vol).cuda(), **kw)
    _same(s, sd, "host source in chunks")
    _same(c, cd, "host source in chunks, cost")
    want = bm.trace(vol, (7, 2, 0, a, 1000, 100), half_width=2, max_step=1, smoothness=0.37)
    _same(s[7:], want[0], "the B-scans at the border")
    _same(c[7:], want[1], "the costs at the border")
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. side effects
def test_tracing_leaves_the_processing_chain_untouched():
    n, a, b = 1024, 64, 2
    p = v180_benchmark_params(n, a, b)
    p.signalGrayscaleMax, p.signalGrayscaleMin = 110.0, 20.0
    p.volumeViewEnabled = p.bscanViewEnabled = p.enFaceViewEnabled = 1
    devs = [_dev(synthetic_raw(n, a, b, seed=180 + k)) for k in range(2)]
    pipe = Pipeline(p, device=0)
    pipe.enable_kernel_timing(True)

    def state():
        pipe.synchronize()
        (pb, nb), (pe, ne) = pipe.display_buffers()
        vp, vn = pipe.volume_view_buffer()
        return (pipe.processed_host(), pipe.mean_line(), _fetch(pb, nb, np.float32), _fetch(pe, ne, np.float32), _fetch(vp, vn, np.uint8))

    pipe.process_device(devs[0].data_ptr())
    before = state()
    launches = pipe.kernel_timing(reset=False)[1]
    host = before[0].reshape(b, a, n // 2).copy()
    for src in (dict(), dict(data=host)):
        s = pipe.trace_boundary(depth=(4, 500), max_step=2, **src)
        pipe.trace_boundary(guide=s, band=(4, 40), cost=True, depth=(4, 500), **src)
        for form in (2, 4):
            pipe.trace_boundary_timed(guide=s, band=(4, 40), depth=(4, 500), form=form, **src)
    assert pipe.kernel_timing(reset=False)[1] == launches
    for x, y in zip(before, state()):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    pipe.process_device(devs[1].data_ptr())
    after = state()
    fresh = Pipeline(p, device=0)
    for d in devs:
        fresh.process_device(d.data_ptr())
        fresh.synchronize()
    assert np.array_equal(after[0].view(np.uint32), fresh.processed_host().view(np.uint32))
    fresh.close()
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 6. the chain
def test_detect_smooth_trace_enface_on_the_device():
    """a bright layer under a tilted entrance surface: detect -> smooth -> trace below the surface -> en face under the traced layer, on
    device tensors from end to end, against the same chain of the two models"""
    n, a, b = 512, 96, 3
    depth = n // 2
    pipe = Pipeline(v180_benchmark_params(n, a, b), device=0)
    rng = np.random.default_rng(15)
    ai, bi = np.meshgrid(np.arange(a), np.arange(b))
    top = np.round(50 + 0.25 * ai + 2 * bi).astype(np.int32)
    layer = top + 30 + np.round(6 * np.sin(ai / 11.0)).astype(np.int32)
    d = np.arange(depth)[None, None, :]
    vol = rng.uniform(0.0, 0.2, (b, a, depth)).astype(np.float32)
    vol += 1.0 * (d >= top[:, :, None]) + 1.5 * (d >= layer[:, :, None])
    vol = vol.astype(np.float32)
    dvol = torch.from_numpy(vol).cuda()
    region = (0, b, 0, a, 8, depth - 8)
    window = dict(depth=region[4:])
    d_raw, d_top, d_layer = (torch.empty((b, a), dtype=torch.int32, device="cuda") for _ in range(3))
    d_image = torch.empty((b, a), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pipe.detect_surface(0.6, 2, data=dvol, out=d_raw, **window)
    pipe.smooth_surface(d_raw, 2, out=d_top)
    got = pipe.trace_boundary(guide=d_top, band=(10, 60), half_width=3, max_step=2, smoothness=0.05, cost=True, data=dvol, out=d_layer, **window)
    assert got[0] is d_layer
    pipe.surface_enface(d_layer, 1, 8, "average", -1.0, data=dvol, out=d_image, **window)
    pipe.synchronize()
    raw = sm.detect(vol, region, 0.6, 2)
    smooth = sm.smooth(raw, 2)
    want, cost = bm.trace(vol, region, guide=smooth, band=(10, 60), half_width=3, max_step=2, smoothness=0.05)
    _same(d_raw.cpu().numpy(), raw, "chain: detect")
    _same(d_top.cpu().numpy(), smooth, "chain: smooth")
    _same(d_layer.cpu().numpy(), want, "chain: trace")
    _same(got[1].cpu().numpy(), cost, "chain: cost")
    _same(d_image.cpu().numpy(), sm.enface(vol, region, want, 1, 8, 0, -1.0), "chain: en face")
    # the host-side chain gives the same bits, and the traced layer is the one that was built
    host = pipe.trace_boundary(guide=pipe.smooth_surface(pipe.detect_surface(0.6, 2, data=vol, **window), 2), band=(10, 60), half_width=3,
                               max_step=2, smoothness=0.05, data=vol, **window)
    _same(host, want, "chain: host side")
    assert np.array_equal(raw, top) and np.array_equal(want, layer)
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------- 7. errors
def test_errors_behind_the_handle(small):
    pipe, vol = small
    for kw, word in ((dict(depth=(0, 129)), "sampleCount"), (dict(ascans=(60, 8)), "ascanCount"), (dict(bscans=(5, 1)), "bscanCount")):
        with pytest.raises(OctPipeError) as e:
            pipe.trace_boundary(data=vol, **kw)
        assert e.value.code == ERR_INVALID_ARGUMENT and word in str(e.value), kw
    with pytest.raises(OctPipeError) as e:
        pipe.trace_boundary_timed(data=vol, depth=(0, 65), form=1)
    assert e.value.code == ERR_INVALID_ARGUMENT and "form" in str(e.value)
    with pytest.raises(ValueError):
        pipe.trace_boundary(guide=np.zeros((5, 66), np.int32), data=vol)
