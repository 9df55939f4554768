"""The eligibility rule of the compute lanes (csrc/lanes.h lane_blockers -- the function every buffer of a live handle goes through)
without a device.  It takes the parameter snapshot, plain facts of the handle (OctPipeLaneFacts) and the kind of the image route; a
buffer goes out on a lane only if NO condition holds.  Every condition is flipped alone against the eligible base case -- the
benchmark's settings on a handle with four slots -- and has to raise its own bit and no other."""
import ctypes as C

import pytest

from octproz_amd import _lib, v180_benchmark_params

# csrc/lanes.h LaneBlocker, in bit order
BITS = ["slots", "host_input", "lut_dirty", "fpn", "sinus", "background", "volume_view", "float_stream", "quant_stream", "callbacks",
        "display_full", "bscan_range", "stream_exposed", "group_member", "scratch_route", "one_lane"]
BIT = {n: 1 << i for i, n in enumerate(BITS)}


def route_of(p, fmt=0, flags=0, fft=1, rtc=1):
    """(kind, prepared, error) of the image launch, from the routing function itself (octpipe_debug_route)"""
    path, kind, intype, roll_w = C.c_uint(), C.c_int(), C.c_int(), C.c_int()
    acq, pod = p.acquisition(), p.pod()
    rc = _lib.lib().octpipe_debug_route(C.byref(acq), C.byref(pod), int(fmt), C.c_uint(flags), int(fft), int(rtc), 0, C.byref(path), C.byref(kind),
                                        C.byref(intype), C.byref(roll_w))
    return kind.value, int(roll_w.value >= 0), int(rc != 0)


def signature(p):
    s = C.c_uint64()
    pod = p.pod()
    assert _lib.lib().octpipe_debug_display_signature(C.byref(pod), C.byref(s)) == 0
    return s.value


def base(N=1024, slots=4):
    """the steady state of the benchmark: device input, calibration done, both views on one frame each, frames extracted before"""
    p = v180_benchmark_params(N, 16, 2, buffers_per_volume=slots)
    p.bscanViewEnabled, p.enFaceViewEnabled = 1, 1
    kind, prepared, error = route_of(p)
    f = _lib.LaneFacts(buffersPerVolume=slots, routeFlags=0, deviceInput=1, lutDirty=0, fpnDetermined=1, meanLinePinned=0,
                       floatStreamingRegistered=0, streamingRegistered=0, callbacksRegistered=0, streamExposed=0, groupMember=0,
                       planKind=kind, planPrepared=prepared, planError=error, lastDisplaySignature=signature(p))
    return p, f


def blockers(p, f):
    b, every = C.c_uint(), C.c_uint()
    pod = p.pod()
    assert _lib.lib().octpipe_debug_lane_blockers(C.byref(f), C.byref(pod), C.byref(b), C.byref(every)) == 0
    assert every.value == (1 << len(BITS)) - 1  # the table above names every condition the library knows
    return b.value


def names(mask):
    return [n for n in BITS if mask & BIT[n]]


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096, 1664])
@pytest.mark.parametrize("slots", [2, 4, 6, 64])
def test_the_steady_state_of_the_benchmark_is_eligible(N, slots):
    p, f = base(N, slots)
    assert names(blockers(p, f)) == []


def _p(**kw):
    def change(p, f):
        for k, v in kw.items():
            setattr(p, k, v)
    return change


def _f(**kw):
    def change(p, f):
        for k, v in kw.items():
            setattr(f, k, v)
    return change


def _both(pk, fk):
    def change(p, f):
        _p(**pk)(p, f)
        _f(**fk)(p, f)
    return change


def _route(flags=0, fmt=0, fft=1, rtc=1, N=None, **settings):
    """the handle's facts follow the routing function for the changed settings (processDeviceRaw asks imagePlan)"""
    def change(p, f):
        if N:
            p.samplesPerLine = N
            p.update_all_curves()
        for k, v in settings.items():
            setattr(p, k, v)
        f.routeFlags = flags
        f.planKind, f.planPrepared, f.planError = route_of(p, fmt, flags, fft, rtc)
        f.lastDisplaySignature = signature(p)
    return change


# (what is flipped, the one bit it must raise)
ROWS = [
    ("one slot", _f(buffersPerVolume=1), "slots"),
    ("three slots", _f(buffersPerVolume=3), "slots"),
    ("63 slots", _f(buffersPerVolume=63), "slots"),
    ("ring / H2D input", _f(deviceInput=0), "host_input"),
    ("tables dirty", _f(lutDirty=1), "lut_dirty"),
    ("mean line not determined yet", _f(fpnDetermined=0), "fpn"),
    ("continuous determination", _p(continuousFixedPatternNoiseDetermination=1), "fpn"),
    ("redetermination requested", _p(redetermineFixedPatternNoise=1), "fpn"),
    ("sinusoidal correction", _p(sinusoidalScanCorrection=1), "sinus"),
    ("background removal", _p(postProcessBackgroundRemoval=1), "background"),
    ("background removal with a recording", _p(postProcessBackgroundRemoval=1, postProcessBackgroundRecordingRequested=1), "background"),
    ("volume view", _p(volumeViewEnabled=1), "volume_view"),
    ("float streaming", _both(dict(streamFloatToHost=1), dict(floatStreamingRegistered=1)), "float_stream"),
    ("quantised streaming", _both(dict(streamToHost=1), dict(streamingRegistered=1)), "quant_stream"),
    ("callbacks", _f(callbacksRegistered=1), "callbacks"),
    ("frames never extracted", _f(lastDisplaySignature=0), "display_full"),
    ("another B-scan on display than extracted", _p(frameNr=1), "display_full"),
    ("another en face plane on display than extracted", _p(frameNrEnFaceView=7), "display_full"),
    ("FULL_DISPLAY route", _f(routeFlags=_lib.ROUTE_FULL_DISPLAY), "display_full"),
    ("B-scan frame averaged over two", _route(functionFramesBscan=2, displayFunctionBscan=0), "bscan_range"),
    ("B-scan frame as a projection over three", _route(functionFramesBscan=3, displayFunctionBscan=1), "bscan_range"),
    ("stream handed out or replaced", _f(streamExposed=1), "stream_exposed"),
    ("group member", _f(groupMember=1), "group_member"),
    ("Lanczos behind the rolling average: prepared rows", _route(resamplingInterpolation=2, backgroundRemoval=1), "scratch_route"),
    ("packed 12-bit rows at N = 256: prepared rows", _route(N=256, fmt=1), "scratch_route"),
    ("library route (N = 600 without the mixed-radix kernels)", _route(N=600, flags=_lib.ROUTE_NO_MIXEDN), "scratch_route"),
    ("run-time compiled kernel (N = 1000)", _route(N=1000), "scratch_route"),
    ("Bluestein (N = 600 without the library)", _route(N=600, flags=_lib.ROUTE_NO_MIXEDN | _lib.ROUTE_NO_LIBFFT, fft=0), "scratch_route"),
    ("no route at all", _f(planKind=0), "scratch_route"),
    ("ONE_LANE route flag", _f(routeFlags=_lib.ROUTE_ONE_LANE), "one_lane"),
]


@pytest.mark.parametrize("what,change,bit", ROWS, ids=[r[0] for r in ROWS])
def test_every_condition_alone_keeps_the_buffer_off_the_lanes(what, change, bit):
    p, f = base()
    change(p, f)
    assert names(blockers(p, f)) == [bit]


# what must NOT block: the other half of each compound condition
FREE = [
    ("mean line pinned, never determined", _f(fpnDetermined=0, meanLinePinned=1)),
    ("mean line pinned, redetermination requested", _both(dict(redetermineFixedPatternNoise=1), dict(meanLinePinned=1))),
    ("no FPN removal, never determined", _both(dict(fixedPatternNoiseRemoval=0), dict(fpnDetermined=0))),
    ("float streaming wanted, no buffers registered", _p(streamFloatToHost=1)),
    ("float buffers registered, streaming off", _f(floatStreamingRegistered=1)),
    ("streaming wanted, no buffers registered", _p(streamToHost=1)),
    ("streaming buffers registered, streaming off", _f(streamingRegistered=1)),
    ("a recording requested with the removal off", _p(postProcessBackgroundRecordingRequested=1)),
    ("both views off, frames never extracted", _both(dict(bscanViewEnabled=0, enFaceViewEnabled=0), dict(lastDisplaySignature=0))),
    ("B-scan view off, its frame count 2", _route(bscanViewEnabled=0, functionFramesBscan=2)),
    ("en face frame averaged over four planes", _route(functionFramesEnFaceView=4, displayFunctionEnFaceView=0)),
    ("other route flags", _route(flags=_lib.ROUTE_TINY_GRID | _lib.ROUTE_NO_REAL_INPUT | _lib.ROUTE_NO_TEAM)),
    ("no dispersion compensation: the real-input kernel", _route(dispersionCompensation=0)),
    ("rolling average inside the kernel", _route(backgroundRemoval=1, rollingAverageWindowSize=8)),
]


@pytest.mark.parametrize("what,change", FREE, ids=[r[0] for r in FREE])
def test_what_does_not_touch_shared_state_stays_eligible(what, change):
    p, f = base()
    change(p, f)
    assert names(blockers(p, f)) == []


def test_conditions_add_up():
    p, f = base()
    _p(sinusoidalScanCorrection=1, volumeViewEnabled=1)(p, f)
    _f(groupMember=1, buffersPerVolume=3)(p, f)
    assert names(blockers(p, f)) == ["slots", "sinus", "volume_view", "group_member"]


def test_the_flag_has_a_bit_of_its_own():
    flags = [getattr(_lib, n) for n in dir(_lib) if n.startswith("ROUTE_")]
    assert len(flags) == len(set(flags))
    assert all(f and f & (f - 1) == 0 for f in flags)
