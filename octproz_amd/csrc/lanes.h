// lanes.h -- WHETHER a buffer may go out on one of the handle's two compute lanes, as one pure function (in the manner of route.h).
//
// A handle has two compute streams: the compute stream itself (lane 0) and a second one (lane 1).  Consecutive buffers of
// octpipe_process_device write different slots of the volume, so in the steady state the whole chain of a buffer -- the transform
// kernel, the display extraction, the timing events -- goes to the lane of its slot's parity, with no event between the lanes: the
// first workgroups of buffer k + 1 take the compute units the last waves of buffer k leave, and the display extraction of k runs
// beside them.  Ordering that needs no stream operation:
//   buffer k and buffer k + buffersPerVolume write the same slot         same parity (buffersPerVolume is even), same lane
//   the display extraction of k reads that slot                          same lane, behind the kernel
//   en-face pixels                                                       every pixel reads its own A-scan: the ranges of different slots are disjoint
//   the B-scan frame, ONE frame on display                               the displayed B-scan lies in one slot: one reading and writing lane
// A B-scan frame that averages or projects SEVERAL B-scans can reach across a slot boundary: the extraction of one slot would read
// B-scans the other lane is writing, and both lanes would write the frame.  Such a display keeps its buffers off the lanes.
// Everything else a buffer can touch is shared by the whole handle (tables, the mean line, scratch rows, the background, the result
// stream's destinations): a buffer that reads while another call may write one of them, or that writes one itself, is NOT eligible
// and runs on the compute stream behind a join of the lanes (octpipe_api.hip joinLanes), like every other entry point of the library.
// The rule is strict on purpose: what it leaves out costs one event pair and runs as it always did.
//
// lane_blockers takes plain facts -- the parameter snapshot, what the handle is and holds (OctPipeLaneFacts, octpipe_debug.h), the
// kind of the image route (route.h) -- and makes no device call: tests/test_lanes.py flips every condition alone in the CPU suite
// (octpipe_debug_lane_blockers).
#pragma once
#include <cstdint>

#include "../../include/octpipe.h"
#include "../../include/octpipe_debug.h"
#include "display_kernels.h"
#include "route.h"

namespace oct {

// what keeps a buffer off the lanes, one bit per condition
enum LaneBlocker : unsigned {
	LANE_BLOCK_SLOTS          = 1u << 0,   // buffersPerVolume is odd or 1: slot parity would not alternate for ever
	LANE_BLOCK_HOST_INPUT     = 1u << 1,   // octpipe_process[_async]: the ring / H2D path orders itself by events on the compute stream
	LANE_BLOCK_LUT_DIRTY      = 1u << 2,   // the look-up tables are uploaded in front of this buffer
	LANE_BLOCK_FPN            = 1u << 3,   // this buffer determines the mean line (lane_fpn_now)
	LANE_BLOCK_SINUS          = 1u << 4,   // sinusoidal scan correction (scratch slot + post pass, or the store-side variant and its fall-back)
	LANE_BLOCK_BACKGROUND     = 1u << 5,   // post-process background removal (with or without a recording: the removal term is rebuilt on the stream)
	LANE_BLOCK_VOLUME_VIEW    = 1u << 6,   // the 8-bit volume view is written behind the chain
	LANE_BLOCK_FLOAT_STREAM   = 1u << 7,   // float streaming to the host (result stream, events, callbacks)
	LANE_BLOCK_QUANT_STREAM   = 1u << 8,   // quantised streaming to the host
	LANE_BLOCK_CALLBACKS      = 1u << 9,   // any callback registered on the handle
	LANE_BLOCK_DISPLAY_FULL   = 1u << 10,  // the display signature has changed (or FULL_DISPLAY): both frames are extracted from the whole volume
	LANE_BLOCK_BSCAN_RANGE    = 1u << 11,  // the B-scan frame is not ONE frame: it may read and be written across a slot boundary
	LANE_BLOCK_STREAM_EXPOSED = 1u << 12,  // octpipe_get_stream / octpipe_set_stream have been called: the caller orders its own work on the stream
	LANE_BLOCK_GROUP_MEMBER   = 1u << 13,  // the handle belongs to an octpipe_group
	LANE_BLOCK_SCRATCH_ROUTE  = 1u << 14,  // the image route writes scratch of the handle (prepared rows, the library route's complex buffer) or may fall back to one that does
	LANE_BLOCK_ONE_LANE       = 1u << 15,  // OCTPIPE_ROUTE_ONE_LANE
	LANE_BLOCK_ALL            = (1u << 16) - 1u
};

// Signature of the display settings: while it is unchanged only the buffer just written can have changed the frames (pipe_display.hip)
inline uint64_t display_signature(const OctPipeParams& p) {
	uint64_t s = 1469598103934665603ull;
	const uint32_t f[] = {(uint32_t)p.bscanViewEnabled, (uint32_t)p.enFaceViewEnabled, p.frameNr, p.functionFramesBscan, (uint32_t)p.displayFunctionBscan,
	                      p.frameNrEnFaceView, p.functionFramesEnFaceView, (uint32_t)p.displayFunctionEnFaceView};
	for (uint32_t v : f) { s ^= v; s *= 1099511628211ull; }
	return s | 1ull;
}

// the buffer that comes next determines the mean line (cu:1518-1525): first buffer, continuous determination, or a request
inline bool lane_fpn_now(const OctPipeLaneFacts& f, const OctPipeParams& p) {
	return p.fixedPatternNoiseRemoval && !f.meanLinePinned &&
	       ((!p.continuousFixedPatternNoiseDetermination && !f.fpnDetermined) || p.continuousFixedPatternNoiseDetermination || p.redetermineFixedPatternNoise);
}

// the transform kernels that read the raw rows and the tables and write nothing but their output; the run-time compiled kernel is
// left out because a failed compilation sends its buffer to a route with scratch (launchFused)
inline bool lane_route_has_scratch(int kind, bool prepared, bool error) {
	return error || prepared || kind <= 0 || kind == ROUTE_KIND_LIBFFT || kind == ROUTE_KIND_BLUESTEIN || kind == ROUTE_KIND_MXS;
}

inline unsigned lane_blockers(const OctPipeLaneFacts& f, const OctPipeParams& p) {
	unsigned b = 0;
	if (f.buffersPerVolume < 2u || (f.buffersPerVolume & 1u)) b |= LANE_BLOCK_SLOTS;
	if (!f.deviceInput) b |= LANE_BLOCK_HOST_INPUT;
	if (f.lutDirty) b |= LANE_BLOCK_LUT_DIRTY;
	if (lane_fpn_now(f, p)) b |= LANE_BLOCK_FPN;
	if (p.sinusoidalScanCorrection) b |= LANE_BLOCK_SINUS;
	if (p.postProcessBackgroundRemoval) b |= LANE_BLOCK_BACKGROUND;  // (a recording happens only with the removal on)
	if (p.volumeViewEnabled) b |= LANE_BLOCK_VOLUME_VIEW;
	if (p.streamFloatToHost && f.floatStreamingRegistered) b |= LANE_BLOCK_FLOAT_STREAM;
	if (p.streamToHost && f.streamingRegistered) b |= LANE_BLOCK_QUANT_STREAM;
	if (f.callbacksRegistered) b |= LANE_BLOCK_CALLBACKS;
	if ((p.bscanViewEnabled || p.enFaceViewEnabled) && (display_signature(p) != f.lastDisplaySignature || (f.routeFlags & OCTPIPE_ROUTE_FULL_DISPLAY))) b |= LANE_BLOCK_DISPLAY_FULL;
	if (p.bscanViewEnabled && display_mode(p.functionFramesBscan, p.displayFunctionBscan) != DISP_SINGLE) b |= LANE_BLOCK_BSCAN_RANGE;
	if (f.streamExposed) b |= LANE_BLOCK_STREAM_EXPOSED;
	if (f.groupMember) b |= LANE_BLOCK_GROUP_MEMBER;
	if (lane_route_has_scratch(f.planKind, f.planPrepared != 0, f.planError != 0)) b |= LANE_BLOCK_SCRATCH_ROUTE;
	if (f.routeFlags & OCTPIPE_ROUTE_ONE_LANE) b |= LANE_BLOCK_ONE_LANE;
	return b;
}
inline bool lane_eligible(const OctPipeLaneFacts& f, const OctPipeParams& p) { return lane_blockers(f, p) == 0u; }
inline int lane_of_slot(unsigned bufferNumberInVolume) { return (int)(bufferNumberInVolume & 1u); }

}  // namespace oct
