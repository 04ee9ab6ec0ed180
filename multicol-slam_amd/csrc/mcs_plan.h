// mcs_plan.h — everything mcs_extractor_create derives from (parameters, image size) before it touches a device: level geometry, FAST cells, slot / dense /
// selection ranges, oct-tree roots, resize taps, mask maps.  Host arithmetic only (mcs_plan.hip makes no HIP call; tests/test_extract_plan_cpu.py runs it alone).
#pragma once
#include "mcs_common.h"
#include <string>
#include <vector>

namespace mcs {

struct ExtractPlan {
	PyrDesc hd{};
	std::vector<CellInfo> cells;    // [hd.cellsPerImage]
	std::vector<ResizeTap> taps;    // x and y tables of levels 1.., then (MCS_PYR_CHAIN) the one-launch chain's region table at hd.chainRegOff
	std::vector<short> maps;        // composed nearest-neighbour maps to level-0 mask coordinates, all levels
};

// MCS_OK and the plan, or the refusal's code with its text in *err.  `p` has passed mcs_extractor_create's parameter checks.
int plan_extractor(const mcs_extractor_params& p, int width, int height, ExtractPlan* plan, std::string* err);

}  // namespace mcs
