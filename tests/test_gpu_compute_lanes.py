"""The two compute lanes of a handle (csrc/lanes.h): consecutive device-resident buffers go to the lane of their slot's parity with
no event between the lanes.  What runs on the lanes must be, bit for bit, what runs on the one compute stream
(OCTPIPE_ROUTE_ONE_LANE): every sequence below runs twice, once per form, and the volume and both display frames are compared at
every snapshot.  octpipe_debug_lane_stats says whether the lanes engaged at all and how often they had to be joined.

All device work happens in ONE child process (this file run as a script prints one JSON record), and inside it every sequence runs
under a time limit of its own (SIGALRM ends the child): a lane join that never completes would otherwise hold the whole suite.
The tests read that record."""
import ctypes as C
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# (samplesPerLine, A-scans, B-scans, extra route flags): the small general kernel on two persistent workgroups, so that every wave
# loops over many A-scans, and the headline kernel
SHAPES = {"n256_tiny_grid": (256, 16, 4, 1024), "n1024": (1024, 8, 2, 0)}
BUFFERS = 9  # distinct seeds per sequence
STEP_LIMIT = 30  # seconds for one sequence in the child (each takes a fraction of a second)
EVENTS = ["synchronize", "copy_processed_to_host", "change_displayed_enface_frame", "lut_dirty", "redetermine_fpn"]
# buffers of a mid-sequence run that go out on a lane: of the first three the very first determines the mean line and extracts both
# frames in full; of the three behind the event all after a wait or a copy, two where the event leaves the next buffer work that is
# not a lane's (full display extraction, table upload, mean line)
EVENT_OVERLAPPED = {"synchronize": 2 + 3, "copy_processed_to_host": 2 + 3, "change_displayed_enface_frame": 2 + 2, "lut_dirty": 2 + 2,
                    "redetermine_fpn": 2 + 2}


# ------------------------------------------------------------------------------------------------ child process
def _child():
    import torch
    sys.path.insert(0, ROOT)
    from octproz_amd import Pipeline, _lib, synthetic_raw, v180_benchmark_params
    hip = C.CDLL("libamdhip64.so")

    def fetch(ptr, nbytes):
        out = np.empty(nbytes, np.uint8)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0
        return out

    def run(shape, slots, one_lane, ops, settings=None):
        """ops: ("buf", i) | ("snap",) | ("stat",) | (event name,) | ("get_stream",) | ("timing_on", stride) | ("timing_read",);
        returns (snapshots, stats)"""
        signal.alarm(STEP_LIMIT)
        N, A, B, flags = SHAPES[shape]
        p = v180_benchmark_params(N, A, B, buffers_per_volume=slots)
        p.bscanViewEnabled, p.enFaceViewEnabled = 1, 1
        p.frameNr, p.frameNrEnFaceView = (B if slots > 1 else 0), N // 8  # a B-scan of slot 1 where there is one
        for k, v in (settings or {}).items():
            setattr(p, k, v)
        pipe = Pipeline(p, device=0, route=flags | (_lib.ROUTE_ONE_LANE if one_lane else 0))
        (pb, nb), (pe, ne) = pipe.display_buffers()
        pv, vbytes, _ = pipe.processed_device()
        snaps, stats = [], []
        for op in ops:
            if op[0] == "buf":
                pipe.process_device(raws[shape][op[1] % BUFFERS].data_ptr(), sync_params=False)
            elif op[0] == "snap":
                pipe.synchronize()
                snaps.append((fetch(pv, vbytes), fetch(pb, 4 * nb), fetch(pe, 4 * ne)))
            elif op[0] == "stat":
                stats.append(pipe.lane_stats())
            elif op[0] == "synchronize":
                pipe.synchronize()
            elif op[0] == "copy_processed_to_host":
                pipe.processed_host(0)
            elif op[0] == "change_displayed_enface_frame":
                pipe.change_displayed_enface_frame(N // 4, 1, 0)
            elif op[0] == "lut_dirty":  # another dispersion curve: the tables are uploaded in front of the next buffer
                p.d2 = -90.0
                p.update_all_curves()
                pipe._sync_params()
            elif op[0] == "redetermine_fpn":
                p.redetermineFixedPatternNoise = 1
                pipe._sync_params()
            elif op[0] == "get_stream":
                pipe.stream_ptr()
            elif op[0] == "timing_on":
                pipe.enable_kernel_timing(True, every=op[1])
            elif op[0] == "timing_read":  # (average ms, timed launches): the count goes into the stats
                stats.append((pipe.kernel_timing()[1], -1))
        pipe.close()
        signal.alarm(0)
        return snaps, stats

    def both(shape, slots, ops, settings=None):
        a, sa = run(shape, slots, False, ops, settings)
        b, sb = run(shape, slots, True, ops, settings)
        bad = [(i, name) for i, (x, y) in enumerate(zip(a, b)) for name, u, v in zip(("volume", "bscan", "enface"), x, y) if not np.array_equal(u, v)]
        return {"snapshots": len(a), "different": bad, "nonzero": all(bool(x[0].any()) and bool(x[2].any()) for x in a), "stats": sa, "stats_one_lane": sb}

    raws = {name: [torch.from_numpy(synthetic_raw(N, A, B, seed=40 + 7 * k).view(np.int16)).to("cuda:0") for k in range(BUFFERS)]
            for name, (N, A, B, _) in SHAPES.items()}
    torch.cuda.synchronize()
    rec = {}
    # bursts of 1, 2, ... 9 buffers, a snapshot behind each: every buffer count's volume and frames, 45 buffers
    bursts = []
    k = 0
    for n in range(1, BUFFERS + 1):
        for _ in range(n):
            bursts.append(("buf", k)); k += 1
        bursts.append(("snap",))
    bursts.append(("stat",))
    for shape in SHAPES:
        for slots in (1, 2, 3, 4):
            rec["bursts/%s/%d" % (shape, slots)] = both(shape, slots, bursts)
    for ev in EVENTS:
        ops = [("buf", 0), ("buf", 1), ("buf", 2), (ev,), ("buf", 3), ("buf", 4), ("buf", 5), ("stat",), ("snap",)]
        rec["event/" + ev] = both("n1024", 4, ops)
    ops = [("buf", 0), ("buf", 1), ("buf", 2), ("stat",), ("get_stream",), ("buf", 3), ("buf", 4), ("buf", 5), ("buf", 6), ("stat",), ("snap",)]
    rec["get_stream"] = both("n256_tiny_grid", 2, ops)
    # a B-scan frame averaged over two B-scans on either side of a slot boundary (the last of slot 0, the first of slot 1): not ONE writing
    # slot, so no buffer of it may go out on a lane
    B = SHAPES["n1024"][2]
    ops = [("buf", k) for k in range(BUFFERS)] + [("stat",), ("snap",)]
    for fn, name in ((0, "average"), (1, "projection")):
        rec["bscan_range/" + name] = both("n1024", 4, ops, dict(frameNr=B - 1, functionFramesBscan=2, displayFunctionBscan=fn))
    # kernel timing with a stride, as the benchmark runs it: every timed launch lands on the same lane (stride 4, four slots) or on both (3)
    for stride in (4, 3):
        ops = [("buf", 0), ("buf", 1), ("timing_on", stride)] + [("buf", k) for k in range(2, 2 + 2 * BUFFERS)] + [("stat",), ("timing_read",), ("stat",), ("snap",)]
        rec["timing/%d" % stride] = both("n1024", 4, ops)
    print(json.dumps(rec))


if __name__ == "__main__":
    _child()
    sys.exit(0)


# ------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def record():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("slots", [2, 4])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_even_slot_counts_overlap_and_write_the_same_bits(record, shape, slots):
    r = record["bursts/%s/%d" % (shape, slots)]
    assert r["snapshots"] == BUFFERS and r["nonzero"]
    assert r["different"] == []
    overlapped, joins = r["stats"][-1]
    # 45 buffers; the first determines the mean line and extracts both frames in full, every other one goes to the lane of its slot
    assert overlapped == 44
    # a burst ends in a wait: joined whenever lane 1 (an odd slot) had work, i.e. in every burst of two or more buffers, and in the
    # bursts of one whose single buffer goes to an odd slot -- only the first burst here, which is the buffer that is not eligible
    assert joins == BUFFERS - 1
    assert r["stats_one_lane"][-1] == [0, 0]


@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_odd_slot_counts_stay_on_the_compute_stream(record, shape, slots):
    r = record["bursts/%s/%d" % (shape, slots)]
    assert r["snapshots"] == BUFFERS and r["nonzero"]
    assert r["different"] == []
    assert r["stats"][-1] == [0, 0] and r["stats_one_lane"][-1] == [0, 0]


@pytest.mark.parametrize("event", EVENTS)
def test_an_entry_point_in_mid_sequence_joins_once_and_changes_nothing(record, event):
    r = record["event/" + event]
    assert r["snapshots"] == 1 and r["nonzero"]
    assert r["different"] == []
    overlapped, joins = r["stats"][-1]
    assert joins == 1  # three buffers in front of it: lane 1 holds one of them
    assert overlapped == EVENT_OVERLAPPED[event]
    assert r["stats_one_lane"][-1] == [0, 0]


def test_a_caller_that_asks_for_the_stream_gets_everything_on_it(record):
    r = record["get_stream"]
    assert r["different"] == [] and r["nonzero"]
    (before, _), (after, joins) = r["stats"]
    assert before == 2 and after == before  # four more buffers behind octpipe_get_stream, none on a lane
    assert joins == 1


@pytest.mark.parametrize("fn", ["average", "projection"])
def test_a_bscan_frame_over_a_slot_boundary_keeps_every_buffer_on_the_compute_stream(record, fn):
    r = record["bscan_range/" + fn]
    assert r["snapshots"] == 1 and r["nonzero"]
    assert r["different"] == []
    assert r["stats"][-1] == [0, 0] and r["stats_one_lane"][-1] == [0, 0]


@pytest.mark.parametrize("stride", [4, 3])
def test_timed_launches_on_the_lanes_change_nothing(record, stride):
    r = record["timing/%d" % stride]
    assert r["snapshots"] == 1 and r["nonzero"]
    assert r["different"] == []
    (overlapped, joins), (launches, _), (_, joins_after) = r["stats"]
    assert overlapped == 1 + 2 * BUFFERS and joins == 0  # 20 buffers, all but the first on a lane, nothing in between
    assert launches == -(-2 * BUFFERS // stride)  # every stride-th of the 18 buffers behind the switch, the first of them included
    assert joins_after == 1  # reading the timings waits for both lanes
    assert r["stats_one_lane"][1][0] == launches
