// plan_driver — prints the extractor plan (csrc/mcs_plan.h) for one parameter set, without a device: tests/test_extract_plan_cpu.py.
//   plan_driver width height nlevels scaleFactor nfeatures useAgast fastAgastType
// First line "rc <code>"; a refusal follows with "err <text>", a plan with one line per record ("hd", "umax", "level", "cell", "tap", "map").
#include "mcs_plan.h"

#include <cstdio>
#include <cstdlib>

namespace mcs {
// The region table of the one-launch resize chain lives beside its kernel (mcs_pyramid.hip) and is reached only with MCS_PYR_CHAIN set, which the test does not do.
bool pyramid_chain_table(const PyrDesc&, const ResizeTap*, std::vector<int>*) { return false; }
}  // namespace mcs

int main(int argc, char** argv) {
	if (argc != 8) { fprintf(stderr, "usage: plan_driver width height nlevels scaleFactor nfeatures useAgast fastAgastType\n"); return 2; }
	mcs_extractor_params p{};
	const int width = atoi(argv[1]), height = atoi(argv[2]);
	p.nlevels = atoi(argv[3]); p.scaleFactor = (float)atof(argv[4]); p.nfeatures = atoi(argv[5]); p.useAgast = atoi(argv[6]); p.fastAgastType = atoi(argv[7]);
	p.edgeThreshold = 25; p.patchSize = 32; p.fastThreshold = 20; p.do_dBrief = 1; p.learnMasks = 1; p.descSize = 32;
	mcs::ExtractPlan plan;
	std::string err;
	const int rc = mcs::plan_extractor(p, width, height, &plan, &err);
	printf("rc %d\n", rc);
	if (rc != MCS_OK) { printf("err %s\n", err.c_str()); return 0; }
	const mcs::PyrDesc& hd = plan.hd;
	printf("hd %d %d %d %d %d %d %d %zu %zu %zu\n", hd.nlevels, hd.kpCap, hd.cellsPerImage, hd.slotsPerImage, hd.densePerImage, hd.selPerImage, hd.pyrBytes,
	       plan.cells.size(), plan.taps.size(), plan.maps.size());
	printf("umax");
	for (int v = 0; v <= mcs::kHalfPatch; ++v) printf(" %d", hd.umax[v]);
	printf("\n");
	for (int l = 0; l < hd.nlevels; ++l) {
		const mcs::LevelInfo& L = hd.lv[l];
		printf("level %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", L.w, L.h, L.nfeat, L.nIni, L.nCols, L.nRows, L.wCell, L.hCell, L.capc, L.cellBase,
		       L.slotBase, L.denseBase, L.denseCap, L.selBase, L.selCap, L.tabX, L.tabY, L.colsOk, L.mapX, L.mapY, L.stride);
	}
	for (const mcs::CellInfo& c : plan.cells) printf("cell %d %d %d %d %d %d\n", c.level, c.x0, c.y0, c.cw, c.ch, c.slot);
	for (const mcs::ResizeTap& t : plan.taps) printf("tap %d %d %d\n", t.ofs, t.a0, t.a1);
	for (short m : plan.maps) printf("map %d\n", m);
	return 0;
}
