// phase_stage_check.cpp -- host check of the staging arithmetic of octpipe_phase_accumulate (octproz_amd/csrc/phase_stage.h), built
// with -fsanitize=address,undefined by tests/test_phase_cases.py.  For rows of 129, 255 and 1024 samples, packed 12 bit and uint16,
// every firstAscan, every ascanCount and several staging budgets, it copies each slice into a heap block of exactly the planned
// staging size (the sanitizer sees any copy or read past either buffer) and then reads the staged rows the way the kernel indexes
// them (csrc/sample_decode.h decode_sample: sample idx of a packed buffer lives in bytes (idx >> 1) * 3 ...), checking that
//   * every wanted row is read exactly once and decodes to the samples the host buffer holds for it,
//   * the bytes read are exactly the bytes copied: from the first wanted row's first byte to the last byte of the copy.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../octproz_amd/csrc/phase_stage.h"

static unsigned sampleOf(size_t row, size_t col) { return (unsigned)((row * 2654435761u + col * 40503u + 17u) & 0xFFFu); }

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAILED %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void run(bool packed, size_t N, size_t lines) {
	const size_t elem = packed ? 0 : 2;
	const size_t S = N * lines;
	const size_t hostBytes = packed ? S / 2 * 3 : S * 2;
	std::vector<uint8_t> hostv(hostBytes);
	uint8_t* host = hostv.data();
	for (size_t r = 0; r < lines; ++r)
		for (size_t c = 0; c < N; ++c) {
			const unsigned v = sampleOf(r, c);
			const size_t idx = r * N + c;
			if (!packed) { host[2 * idx] = (uint8_t)v; host[2 * idx + 1] = (uint8_t)(v >> 8); continue; }
			uint8_t* b = host + (idx >> 1) * 3;
			if (idx & 1) { b[1] = (uint8_t)((b[1] & 0x0F) | ((v & 0xF) << 4)); b[2] = (uint8_t)(v >> 4); }
			else { b[0] = (uint8_t)v; b[1] = (uint8_t)((b[1] & 0xF0) | (v >> 8)); }
		}
	const size_t oneRow = oct::phase_stage_row_bytes(packed, N, elem, 1);
	const size_t budgets[] = {1, oneRow, 2 * oneRow, 3 * oneRow + 1, 5 * oneRow, (size_t)64 << 20};
	for (size_t budget : budgets)
		for (size_t first = 0; first < lines; ++first)
			for (size_t count = 1; first + count <= lines; ++count) {
				const oct::PhaseStagePlan p = oct::phase_stage_plan(packed, N, elem, first, count, budget);
				std::vector<int> seen(lines, 0);
				for (size_t i = 0; i < p.slices; ++i) {
					const oct::PhaseStageSlice s = oct::phase_stage_slice(p, packed, N, elem, first, count, i);
					CHECK(s.bytes <= p.stageBytes && s.srcByte + s.bytes <= hostBytes && s.rows >= 1, "N %zu first %zu count %zu budget %zu slice %zu", N, first, count, budget, i);
					if (fails) return;
					uint8_t* stage = new uint8_t[p.stageBytes];  // exactly what grow() is asked for
					memcpy(stage, host + s.srcByte, s.bytes);
					size_t lo = (size_t)-1, hi = 0;
					for (size_t row = s.firstRow; row < s.firstRow + s.rows; ++row) {
						const size_t global = first - p.lead + i * p.sliceRows + row;
						CHECK(global < lines, "row %zu", global);
						if (global >= lines) return;
						seen[global]++;
						for (size_t c = 0; c < N; ++c) {
							const size_t idx = row * N + c;
							unsigned v;
							size_t b0, b1;
							if (packed) {
								const size_t t = (idx >> 1) * 3;
								b0 = (idx & 1) ? t + 1 : t;
								b1 = b0 + 1;
								v = (idx & 1) ? ((unsigned)stage[t + 1] >> 4) | ((unsigned)stage[t + 2] << 4) : (unsigned)stage[t] | (((unsigned)stage[t + 1] & 15u) << 8);
							} else {
								b0 = 2 * idx;
								b1 = b0 + 1;
								v = (unsigned)stage[b0] | ((unsigned)stage[b1] << 8);
							}
							CHECK(b1 < s.bytes, "byte %zu of %zu copied", b1, s.bytes);
							CHECK(v == sampleOf(global, c), "N %zu first %zu count %zu budget %zu: row %zu col %zu", N, first, count, budget, global, c);
							if (b0 < lo) lo = b0;
							if (b1 > hi) hi = b1;
						}
					}
					const size_t wantLo = packed ? ((s.firstRow * N) >> 1) * 3 + ((s.firstRow * N) & 1) : s.firstRow * N * 2;
					CHECK(lo == wantLo && hi == s.bytes - 1, "N %zu first %zu count %zu budget %zu slice %zu: read [%zu, %zu] of %zu copied", N, first, count, budget, i, lo, hi, s.bytes);
					delete[] stage;
				}
				for (size_t r = 0; r < lines; ++r)
					CHECK(seen[r] == (r >= first && r < first + count ? 1 : 0), "N %zu first %zu count %zu budget %zu: row %zu read %d times", N, first, count, budget, r, seen[r]);
			}
}

int main() {
	for (size_t N : {(size_t)129, (size_t)255, (size_t)1024}) {
		run(true, N, 8);
		run(true, N, 6);
		run(false, N, 5);
	}
	// the rule before the fix, for the record: rows cut at firstAscan * floor(1.5 N) start one byte late at N = 129, firstAscan = 1
	const size_t N = 129, wrong = 1 * (N * 8 / 2 * 3 / 8), right = ((1 * N) >> 1) * 3;
	printf("N = 129, firstAscan = 1: row starts in byte %zu (odd sample of its pair), floor(1.5 N) = %zu\n", right, wrong);
	if (fails) { printf("%d checks failed\n", fails); return 1; }
	printf("phase staging: all checks passed\n");
	return 0;
}
