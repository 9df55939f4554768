// sample_decode.h -- the bit-level decode of one raw sample (include/octpipe.h "sample formats"), shared by the float decode of the
// processing chain (side_kernels.h prepare_decode), the integer accumulation of the phase extraction (phase_extract.h) and the raw
// statistics (image_stats.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

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

// The eight raw containers as the integer kernels template them (phase_extract.h, image_stats.h), then the processed float32 source
// of the calls that read either (image_stats.h, pipe_region.hip)
enum { PH_U8, PH_U16, PH_U32, PH_P12U, PH_P12S, PH_I8, PH_I16, PH_I32, PH_COUNT, ST_F32 = PH_COUNT, ST_COUNT };
template <int F> struct PhFmt;
// bitDepth / format as decode_sample takes them; V samples per vector load of CHUNK bytes; WIDE: 32-bit samples, int64 lane sums
template <> struct PhFmt<PH_U8>   { static constexpr int BD = 8,  FMT = 0, V = 16, CHUNK = 16; static constexpr bool WIDE = false; };
template <> struct PhFmt<PH_U16>  { static constexpr int BD = 16, FMT = 0, V = 8,  CHUNK = 16; static constexpr bool WIDE = false; };
template <> struct PhFmt<PH_U32>  { static constexpr int BD = 32, FMT = 0, V = 4,  CHUNK = 16; static constexpr bool WIDE = true; };
template <> struct PhFmt<PH_P12U> { static constexpr int BD = 12, FMT = 1, V = 8,  CHUNK = 12; static constexpr bool WIDE = false; };
template <> struct PhFmt<PH_P12S> { static constexpr int BD = 12, FMT = 2, V = 8,  CHUNK = 12; static constexpr bool WIDE = false; };
template <> struct PhFmt<PH_I8>   { static constexpr int BD = 8,  FMT = 3, V = 16, CHUNK = 16; static constexpr bool WIDE = false; };
template <> struct PhFmt<PH_I16>  { static constexpr int BD = 16, FMT = 4, V = 8,  CHUNK = 16; static constexpr bool WIDE = false; };
template <> struct PhFmt<PH_I32>  { static constexpr int BD = 32, FMT = 5, V = 4,  CHUNK = 16; static constexpr bool WIDE = true; };
template <> struct PhFmt<ST_F32>  { static constexpr int BD = 32, V = 4, CHUNK = 16; };  // (no integer decode: decode_sample never sees it)

// f(std::integral_constant<int, F>()) for the one F in [0, COUNT) that equals fmt (COUNT: PH_COUNT or ST_COUNT); `other` for any other value
template <int COUNT, int F = 0, class R, class Fn> R with_format(int fmt, R other, Fn f) {
	if constexpr (F < COUNT) return fmt == F ? f(std::integral_constant<int, F>()) : with_format<COUNT, F + 1>(fmt, other, f);
	else return other;
}
// what the host needs to know of a container: samples per vector load, packed 12 bit or not, bytes per element (packed: 0, 1.5 in truth)
inline unsigned format_vector(int fmt) { return with_format<ST_COUNT>(fmt, 0u, [](auto F) { return (unsigned)PhFmt<F()>::V; }); }
inline bool format_packed(int fmt) { return with_format<ST_COUNT>(fmt, false, [](auto F) { return PhFmt<F()>::BD == 12; }); }
inline size_t format_elem_bytes(int fmt) { return format_packed(fmt) ? 0 : with_format<ST_COUNT>(fmt, (size_t)0, [](auto F) { return (size_t)PhFmt<F()>::BD / 8; }); }

// PH_* of a handle's sample format (OCTPIPE_FORMAT_*) and bit depth
inline int ph_format(int sampleFormat, unsigned bitDepth) {
	switch (sampleFormat) {
	case 1: return PH_P12U;
	case 2: return PH_P12S;
	case 3: return PH_I8;
	case 4: return PH_I16;
	case 5: return PH_I32;
	default: return bitDepth <= 8 ? PH_U8 : bitDepth <= 16 ? PH_U16 : PH_U32;
	}
}

}  // namespace oct
