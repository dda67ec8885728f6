#include "filterplan.h"

#include <algorithm>
#include <cmath>

namespace TwoPaCo
{
	double HllEstimate(const uint8_t * registers, size_t m)
	{
		double sum = 0;
		size_t zeros = 0;
		for (size_t i = 0; i < m; i++)
		{
			sum += std::ldexp(1.0, -int(registers[i]));
			zeros += registers[i] == 0;
		}

		if (m == 0 || zeros == m) return 0;
		const double dm = double(m);
		const double alpha = 0.7213 / (1.0 + 1.079 / dm);
		const double estimate = alpha * dm * dm / sum;
		if (estimate <= 2.5 * dm && zeros > 0) return dm * std::log(dm / double(zeros));
		return estimate;
	}

	double PredictedFalseMarks(double distinctEdges, unsigned hashFunctions, unsigned filterBits, unsigned rounds)
	{
		const double perRound = distinctEdges / double(std::max(1u, rounds));
		const double fill = -std::expm1(-double(hashFunctions) * perRound / std::ldexp(1.0, int(filterBits)));
		return 6.0 * std::pow(fill, double(hashFunctions));
	}

	FilterPlan PlanFilter(uint64_t distinctEdges, unsigned hashFunctions, uint64_t textLength, uint64_t filterBytesCap, unsigned userRounds)
	{
		const double n = double(std::min(distinctEdges, textLength));
		const unsigned q = std::max(1u, hashFunctions);
		FilterPlan plan;
		plan.rounds = std::max(1u, userRounds);
		plan.bitsForTarget = FILTER_PLAN_MIN_BITS;
		while (plan.bitsForTarget < 62 && PredictedFalseMarks(n, q, plan.bitsForTarget, plan.rounds) > FILTER_PLAN_TARGET) ++plan.bitsForTarget;
		plan.bitsForMemory = FILTER_PLAN_MIN_BITS;
		while (plan.bitsForMemory < FILTER_PLAN_MAX_BITS && (uint64_t(1) << (plan.bitsForMemory + 1)) / 8 <= filterBytesCap) ++plan.bitsForMemory;
		plan.filterBits = std::min(plan.bitsForMemory, std::max(plan.bitsForTarget, FILTER_PLAN_FLOOR));
		if (userRounds == 0 && plan.bitsForTarget > plan.bitsForMemory)
		{
			while (plan.rounds < FILTER_PLAN_MAX_ROUNDS && PredictedFalseMarks(n, q, plan.filterBits, plan.rounds) > FILTER_PLAN_TARGET) ++plan.rounds;
		}

		plan.falseMarks = PredictedFalseMarks(n, q, plan.filterBits, plan.rounds);
		plan.clipped = plan.falseMarks > FILTER_PLAN_TARGET;
		return plan;
	}
}
