// sample_decode.h -- the bit-level decode of one raw sample (include/octpipe.h "sample formats"), shared by the float decode of the
// processing chain (side_kernels.h prepare_decode) and the integer accumulation of the phase extraction (phase_extract.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_regs.h"

namespace oct {

// Sample idx of `raw` as its stored integer with the >> 4 of bitshift applied (arithmetic for the signed formats), handed to `conv`
// as an int (signed formats) or a uint32_t (unsigned ones).  32-bit unsigned samples (format 0, bitDepth > 16) go to `u32` as
// stored: the float route scales them by 2^-32 under bitshift instead of shifting.  format: OCTPIPE_FORMAT_* (0 = by bit depth as
// the reference cu:109-147; 1/2 packed 12 bit, 3/4/5 signed).
template <class Conv, class U32>
OCT_DEV auto decode_sample(const void* raw, size_t idx, int bitDepth, int bitshift, int format, Conv conv, U32 u32) {
	if (format == 1 || format == 2) {
		// samples 2p, 2p+1 live in bytes 3p .. 3p+2
		const uint8_t* b = reinterpret_cast<const uint8_t*>(raw) + (idx >> 1) * 3;
		const uint32_t v = (idx & 1) ? ((uint32_t)b[1] >> 4) | ((uint32_t)b[2] << 4) : (uint32_t)b[0] | (((uint32_t)b[1] & 15u) << 8);
		if (format == 1) return conv(bitshift ? (v >> 4) : v);
		const int sv = (int)(v << 20) >> 20;  // sign-extend 12 bits
		return conv(bitshift ? (sv >> 4) : sv);
	}
	if (format == 3) { const int v = reinterpret_cast<const int8_t*>(raw)[idx]; return conv(bitshift ? (v >> 4) : v); }
	if (format == 4) { const int v = reinterpret_cast<const int16_t*>(raw)[idx]; return conv(bitshift ? (v >> 4) : v); }
	if (format == 5) { const int v = reinterpret_cast<const int32_t*>(raw)[idx]; return conv(bitshift ? (v >> 4) : v); }
	if (bitDepth <= 8) { uint32_t v = reinterpret_cast<const uint8_t*>(raw)[idx]; return conv(bitshift ? (v >> 4) : v); }
	if (bitDepth <= 16) { uint32_t v = reinterpret_cast<const uint16_t*>(raw)[idx]; return conv(bitshift ? (v >> 4) : v); }
	uint32_t v = reinterpret_cast<const uint32_t*>(raw)[idx];
	return u32(v);
}

}  // namespace oct
