// filterplan.h -- `twopaco -f auto`: from the HyperLogLog registers of the distinct canonical (k+1)-mers (the device's
// tpc_distinct_sketch, include/twopaco_hip.h) to a count, and from the count to the Bloom filter size 2^L and the number of
// rounds.  Plain arithmetic: no device, no file.  The reference has no counterpart (its README gives a rule of thumb keyed to
// the host's RAM); DESIGN.md has the model and the two sweep points it was checked against.
#ifndef _FILTER_PLAN_H_
#define _FILTER_PLAN_H_

#include <cstddef>
#include <cstdint>

namespace TwoPaCo
{
	const size_t HLL_REGISTERS = 16384;  // p = 14

	// The HyperLogLog estimate of m one-byte registers: alpha m^2 / sum 2^-reg with alpha = 0.7213 / (1 + 1.079 / m), replaced by
	// linear counting m ln(m / V) when it is at most 2.5 m and V > 0 registers are zero.  The hash has 64 bits: no large-range
	// correction.  All-zero registers give 0.
	double HllEstimate(const uint8_t * registers, size_t m);

	// False marks the model predicts per text position: a position that is no junction probes six absent edges, each of which
	// passes with the filter's fill to the q-th power, fill = 1 - exp(-q (n / r) / 2^L) for n distinct edges cut over r rounds.
	double PredictedFalseMarks(double distinctEdges, unsigned hashFunctions, unsigned filterBits, unsigned rounds);

	// A further 0.1 % of the positions marked by mistake adds under 1 % to the second pass's work on the 62-genome workload, whose
	// real marks are 14 % of its positions (44.0 M of 309.5 M, profiles/r04s_f_sweep.json).
	const double FILTER_PLAN_TARGET = 1e-3;
	// Below this the query takes a slower path whatever the false-positive rate (81 ms at L = 30 against 26 ms at 32 on the
	// 62-genome step: profiles/r04s_f_sweep.json, profiles/r05_f_sweep.json).  Re-measured by tools/auto_filter_bench.py,
	// profiles/auto_filter.json: 38.6 ms at 30, 25.05 at 32, 23.97 at 34, best 23.95 at 35 -- the "beyond spread" rule gives 34
	// there (32 is 4.6 % behind the best).  Kept at 32: one sweep on one box, and a floor of 34 quadruples what every small input
	// allocates and zeroes (DESIGN.md 3.6 records it as open).
	const unsigned FILTER_PLAN_FLOOR = 32;
	const unsigned FILTER_PLAN_MAX_BITS = 40;    // the largest filter the project runs (tests/test_gpu_big.py)
	const unsigned FILTER_PLAN_MIN_BITS = 3;     // one byte
	const unsigned FILTER_PLAN_MAX_ROUNDS = 64;  // an arbitrary stop: beyond it the plan keeps 64 rounds and says `clipped`

	struct FilterPlan
	{
		unsigned filterBits;     // L
		unsigned rounds;         // r: the caller's, or the plan's choice
		double falseMarks;       // PredictedFalseMarks at (L, r)
		bool clipped;            // the target is not met at (L, r): memory clips L and the rounds (the caller's, or 64) do not make up for it
		unsigned bitsForTarget;  // L_fp: the smallest L that meets the target with the rounds in use (the caller's, or one)
		unsigned bitsForMemory;  // L_mem: the largest L with 2^L / 8 <= filterBytesCap, at most FILTER_PLAN_MAX_BITS
	};

	// L = min(L_mem, max(L_fp, FILTER_PLAN_FLOOR)).  userRounds = 0: the plan chooses -- one round, or, when L_fp > L_mem, the
	// smallest r <= FILTER_PLAN_MAX_ROUNDS that meets the target at L_mem.  distinctEdges is clamped to textLength (an estimate
	// cannot exceed the number of windows).
	FilterPlan PlanFilter(uint64_t distinctEdges, unsigned hashFunctions, uint64_t textLength, uint64_t filterBytesCap, unsigned userRounds);
}

#endif
