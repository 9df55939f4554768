// phase_stage.h -- which bytes of a host raw buffer octpipe_phase_accumulate stages for a run of A-scans (pipe_phase.hip), in plain
// C++ so that a host program can check it (tests/native/phase_stage_check.cpp).
//
// A row of N samples is N * elemBytes bytes, and row r starts at byte r * N * elemBytes.  Packed 12 bit is different when N is odd: two
// samples share a byte triple, so row r starts at byte ((r * N) >> 1) * 3 and, when r * N is odd, in the middle of a triple.  Only
// the even rows start a triple (2k * N samples are k * N triples).  The staged range therefore begins at the even row at or below the
// first wanted row, the kernel skips that `lead` row through firstRow, every slice holds an even number of rows so that the next one
// begins on an even row again, and the byte count is rounded up: the last sample of an odd run of samples takes the first two bytes
// of its triple.
#pragma once
#include <stddef.h>

namespace oct {

struct PhaseStagePlan {
	size_t lead;       // rows in front of the first wanted one that travel with it (0 or 1)
	size_t sliceRows;  // staged rows per slice, the lead row included
	size_t slices;
	size_t stageBytes; // size of the staging buffer: the largest slice
};

struct PhaseStageSlice {
	size_t srcByte, bytes;  // the copy: host bytes [srcByte, srcByte + bytes) to byte 0 of the staging buffer
	size_t firstRow, rows;  // what the kernel sums of the staged rows
};

inline bool phase_stage_split_rows(bool packed, size_t N) { return packed && (N & 1); }

// bytes of `rows` rows that start on a row boundary which is also a byte (packed: triple) boundary
inline size_t phase_stage_row_bytes(bool packed, size_t N, size_t elemBytes, size_t rows) {
	return packed ? (rows * N * 3 + 1) / 2 : rows * N * elemBytes;
}

inline PhaseStagePlan phase_stage_plan(bool packed, size_t N, size_t elemBytes, size_t firstAscan, size_t ascanCount, size_t budgetBytes) {
	PhaseStagePlan p;
	const bool split = phase_stage_split_rows(packed, N);
	p.lead = split ? (firstAscan & 1) : 0;
	size_t sliceRows = budgetBytes / phase_stage_row_bytes(packed, N, elemBytes, 1);
	if (split) sliceRows &= ~(size_t)1;
	if (sliceRows < (split ? 2u : 1u)) sliceRows = split ? 2 : 1;
	const size_t total = p.lead + ascanCount;
	p.sliceRows = sliceRows;
	p.slices = (total + sliceRows - 1) / sliceRows;
	p.stageBytes = phase_stage_row_bytes(packed, N, elemBytes, total < sliceRows ? total : sliceRows);
	return p;
}

inline PhaseStageSlice phase_stage_slice(const PhaseStagePlan& p, bool packed, size_t N, size_t elemBytes, size_t firstAscan, size_t ascanCount, size_t i) {
	const size_t total = p.lead + ascanCount;
	const size_t r0 = firstAscan - p.lead + i * p.sliceRows;  // even whenever rows can start inside a triple
	const size_t n = total - i * p.sliceRows < p.sliceRows ? total - i * p.sliceRows : p.sliceRows;
	PhaseStageSlice s;
	s.srcByte = packed ? r0 * N / 2 * 3 : r0 * N * elemBytes;
	s.bytes = phase_stage_row_bytes(packed, N, elemBytes, n);
	s.firstRow = i == 0 ? p.lead : 0;
	s.rows = n - s.firstRow;
	return s;
}

}  // namespace oct
