// mcs_plan.hip — the extractor's host-side tables in the reference's exact float / double steps (mcs_plan.h).  No HIP call in this file.
#include "mcs_plan.h"
#include "mcs_host.h"

#include <cstdlib>

namespace mcs {

static void build_umax(int* umax) {   // reference src/mdBRIEFextractorOct.cpp:187-202
	int v, v0, vmax = cvFloor_(kHalfPatch * sqrt(2.f) / 2 + 1);
	int vmin = (int)ceil(kHalfPatch * sqrt(2.f) / 2);
	const double hp2 = kHalfPatch * kHalfPatch;
	for (v = 0; v <= kHalfPatch; ++v) umax[v] = 0;
	for (v = 0; v <= vmax; ++v) umax[v] = cvRound_(sqrt(hp2 - v * v));
	for (v = kHalfPatch, v0 = 0; v >= vmin; --v) {
		while (umax[v0] == umax[v0 + 1]) ++v0;
		umax[v] = v0;
		++v0;
	}
}

int plan_extractor(const mcs_extractor_params& p, int width, int height, ExtractPlan* plan, std::string* err) {
	auto refuse = [&](int code, const char* msg) { *err = msg; return code; };
	*plan = ExtractPlan{};
	PyrDesc& hd = plan->hd;
	std::vector<ResizeTap>& taps = plan->taps;
	std::vector<short>& maps = plan->maps;
	const int nl = p.nlevels;
	hd.nlevels = nl; hd.width = width; hd.height = height;
	hd.fastThreshold = std::min(std::max(p.fastThreshold, 0), 255);
	hd.fastRing = p.fastAgastType == 2 ? 16 : (p.fastAgastType == 1 ? 12 : 8);
	hd.agast = p.useAgast ? p.fastAgastType : -1;
	// border of the detector inside a cell view: cv::FAST keeps 3 pixels for every ring, cv::AGAST the ring's radius (1 / 3 / 2 / 3)
	const int detB = !p.useAgast ? 3 : (p.fastAgastType == 0 ? 1 : (p.fastAgastType == 2 ? 2 : 3));
	hd.descSize = p.descSize; hd.npoints = 2 * 8 * p.descSize;
	hd.mode = p.learnMasks ? 2 : (p.do_dBrief ? 1 : 0);
	hd.undistort = p.do_dBrief ? 1 : 0;

	// scale tables in double from the FLOAT scale factor (ctor :153-179)
	std::vector<double> sc(nl, 1.0), inv(nl, 1.0);
	const double scaleFactor = p.scaleFactor;
	for (int i = 1; i < nl; i++) sc[i] = sc[i - 1] * scaleFactor;
	const double invScaleFactor = 1.0 / scaleFactor;
	for (int i = 1; i < nl; i++) inv[i] = inv[i - 1] * invScaleFactor;
	std::vector<int> nfeat(nl);
	{
		double factor = (1.0 / scaleFactor);
		double nDesired = p.nfeatures * (1 - factor) / (1 - pow(factor, nl));
		int sum = 0;
		for (int level = 0; level < nl - 1; level++) { nfeat[level] = cvRound_(nDesired); sum += nfeat[level]; nDesired *= factor; }
		nfeat[nl - 1] = std::max(p.nfeatures - sum, 0);
	}

	int off = 0, cellBase = 0, slotBase = 0, denseBase = 0, selBase = 0;
	for (int l = 0; l < nl; ++l) {
		LevelInfo& L = hd.lv[l];
		L.w = cvRound_((double)width * inv[l]);
		L.h = cvRound_((double)height * inv[l]);
		L.stride = (L.w + 63) / 64 * 64;
		L.off = off;
		off += L.stride * L.h;
		const int minB = kMinBorder, maxBX = L.w - kEdge + 3, maxBY = L.h - kEdge + 3;
		const double wd = (maxBX - minB), ht = (maxBY - minB);
		L.nCols = (int)(wd / (double)kCellW);
		L.nRows = (int)(ht / (double)kCellW);
		if (wd < 1 || ht < 1 || (l == 0 && (L.nCols < 1 || L.nRows < 1)) || L.w - 2 * kMinBorder >= 4096 || L.h - 2 * kMinBorder >= 4096)
			return refuse(MCS_ERR_UNSUPPORTED, "image too small for the requested number of levels (a level is narrower than its 44-px border, or level 0 has no 30-px FAST cell) or too large");
		// A level whose inner region is less than one 30-px cell high or wide: the reference's cell loops do not run (nRows or nCols = 0, :886-887), the oct-tree gets no
		// keys and the level contributes nothing — an EMPTY level here (no cells, no slots); everything else about it (resize, blur, the feature budget) stays
		const bool emptyLevel = L.nCols < 1 || L.nRows < 1;
		if (emptyLevel) { L.nCols = L.nRows = 0; L.wCell = L.hCell = 0; L.capc = 0; }
		else {
			L.wCell = (int)ceil(wd / L.nCols);
			L.hCell = (int)ceil(ht / L.nRows);
			L.capc = p.useAgast ? ((L.wCell + 6 - 2 * detB) * (L.hCell + 6 - 2 * detB) + 1) / 2 : ((L.wCell + 1) / 2) * ((L.hCell + 1) / 2);
		}
		L.cellBase = cellBase; L.slotBase = slotBase;
		for (int i = 0; i < L.nRows; i++)
			for (int j = 0; j < L.nCols; j++) {
				CellInfo c{};
				c.level = (short)l;
				const double iniY = minB + i * L.hCell, iniX = minB + j * L.wCell;
				double maxY = iniY + L.hCell + 6, maxX = iniX + L.wCell + 6;
				bool skip = (iniY >= maxBY - 3) || (iniX >= maxBX - 6);   // :897,906
				if (maxY > maxBY) maxY = maxBY;
				if (maxX > maxBX) maxX = maxBX;
				c.x0 = (short)(iniX + detB); c.y0 = (short)(iniY + detB);
				c.cw = skip ? 0 : (short)std::max(0, (int)maxX - (int)iniX - 2 * detB);
				c.ch = skip ? 0 : (short)std::max(0, (int)maxY - (int)iniY - 2 * detB);
				c.slot = slotBase + (i * L.nCols + j) * L.capc;
				{   // k_fast_cells: tile row = cw + 4 + 3 bytes in dwords
					const int ndw = (c.cw + 4 + 3 + 3) >> 2;
					c.rowM = (65536 + ndw - 1) / ndw;
				}
				plan->cells.push_back(c);
			}
		cellBase += L.nCols * L.nRows;
		slotBase += L.nCols * L.nRows * L.capc;
		L.denseBase = denseBase; L.denseCap = L.nCols * L.nRows * L.capc;
		denseBase += L.denseCap;
		L.nfeat = nfeat[l];
		L.selBase = selBase; L.selCap = std::max(L.nfeat + 3, 4 * kMaxRoots);
		selBase += L.selCap;
		// oct-tree roots (:641-661)
		L.nIni = cvRound_(wd / ht);
		if (L.nIni > kMaxRoots || L.nfeat + 3 > kMaxNodes)
			return refuse(MCS_ERR_UNSUPPORTED, "aspect ratio / features per level outside the oct-tree kernel's capacity (nIni <= 32, nfeatures_level+3 <= 2048)");
		// nIni = 0 (a level more than twice as tall as wide, e.g. the small top levels of a portrait image): the reference divides by it and, as soon as the level has a
		// candidate, indexes an empty root vector (:641-661, undefined).  Its only defined outcome — a level without candidates — is "no keypoint on this level", and that
		// is what such a level yields here whatever it holds (tests/test_gpu_extract.py::test_portrait_levels_without_an_octree_root).
		if (L.nIni < 1) L.nIni = 0;
		L.hX = L.nIni > 0 ? wd / L.nIni : wd;
		for (int i = 0; i <= L.nIni; ++i) L.rootX[i] = (int)(L.hX * static_cast<double>(i));
		L.scale = (float)sc[l];
		L.kpSize = (float)(int)(kPatchSize * sc[l]);
		// resize tables from level l-1 (cv::resize INTER_LINEAR, Appendix A.1) and composed nearest-neighbour maps (A.2)
		L.tabX = (int)taps.size();
		if (l > 0) {
			const LevelInfo& P = hd.lv[l - 1];
			const double scale_x = 1. / ((double)L.w / P.w), scale_y = 1. / ((double)L.h / P.h);
			for (int dx = 0; dx < L.w; dx++) {
				float fx = (float)((dx + 0.5) * scale_x - 0.5);
				int sx = cvFloor_(fx);
				fx -= sx;
				if (sx < 0) { fx = 0; sx = 0; }
				if (sx >= P.w - 1) { fx = 0; sx = P.w - 1; }
				ResizeTap t{(short)sx, sat_short((1.f - fx) * 2048), sat_short(fx * 2048), 0};
				taps.push_back(t);
			}
			// k_resize_cols: every group of four adjacent columns must read within 8 adjacent source bytes (any scale factor up to 2), rows per thread <= 64
			L.colsOk = P.w >= 8 && L.h >= 1;
			for (int dx = 0; dx < L.w; dx += 4)
				if (taps[L.tabX + std::min(dx + 3, L.w - 1)].ofs - taps[L.tabX + dx].ofs > 6) L.colsOk = 0;
			L.tabY = (int)taps.size();
			for (int dy = 0; dy < L.h; dy++) {
				float fy = (float)((dy + 0.5) * scale_y - 0.5);
				int sy = cvFloor_(fy);
				fy -= sy;
				ResizeTap t{(short)sy, sat_short((1.f - fy) * 2048), sat_short(fy * 2048), 0};
				taps.push_back(t);
			}
		} else { L.tabY = L.tabX; L.colsOk = 0; }
		L.mapX = (int)maps.size();
		for (int x = 0; x < L.w; ++x) {
			if (l == 0) maps.push_back((short)x);
			else {
				const LevelInfo& P = hd.lv[l - 1];
				const double ifx = 1. / ((double)L.w / P.w);
				maps.push_back(maps[P.mapX + std::min(cvFloor_(x * ifx), P.w - 1)]);
			}
		}
		L.mapY = (int)maps.size();
		for (int y = 0; y < L.h; ++y) {
			if (l == 0) maps.push_back((short)y);
			else {
				const LevelInfo& P = hd.lv[l - 1];
				const double ify = 1. / ((double)L.h / P.h);
				maps.push_back(maps[P.mapY + std::min(cvFloor_(y * ify), P.h - 1)]);
			}
		}
	}
	hd.pyrBytes = off;
	hd.cellsPerImage = cellBase; hd.slotsPerImage = slotBase; hd.densePerImage = denseBase; hd.selPerImage = selBase;
	// rows per image: DistributeOctTree returns at most nfeat_l + 3 keys for a level (a split adds <= 3 nodes before the `>= N` test) — but its first
	// expansion pass runs before that test, so a level can also return up to 4 * nIni keys whatever its quota (:663-700)
	hd.kpCap = 0;
	for (int l = 0; l < nl; ++l) hd.kpCap += std::max(hd.lv[l].nfeat + 3, 4 * hd.lv[l].nIni);

	// orientation disc (IC_Angle rows v = 0, +-1..+-16 with |u| <= umax[|v|], 845 pixels)
	int umax[kHalfPatch + 1];
	build_umax(umax);
	std::vector<signed char> disc;
	for (int v = -kHalfPatch; v <= kHalfPatch; ++v)
		for (int u = -umax[std::abs(v)]; u <= umax[std::abs(v)]; ++u) { disc.push_back((signed char)u); disc.push_back((signed char)v); }
	if (disc.size() != 845 * 2) return refuse(MCS_ERR_INVALID, "internal: disc size");
	for (int v = 0; v <= kHalfPatch; ++v) hd.umax[v] = umax[v];

	hd.chainFits = 0; hd.chainRegOff = 0;
	// One launch for the whole resize chain (k_resize_chain, bit-exact, tests/test_gpu_env_paths.py) is opt-in: measured 0.37 ms alone against 0.22 ms for the
	// seven launches (its 6912 workgroups pay eight barriers and the small levels run at a quarter of the lanes), default step 2.20 against 2.09 ms.
	// (Also measured without gain on the seven-launch chain: FAST launched per level as soon as the level exists, 2.11 ms.)
	if (getenv("MCS_PYR_CHAIN") && !taps.empty()) {
		std::vector<int> table;
		if (pyramid_chain_table(hd, taps.data(), &table)) {   // regions of the one-launch resize chain, stored behind the taps (8 bytes per entry)
			hd.chainFits = 1; hd.chainRegOff = (int)taps.size();
			taps.resize(taps.size() + (table.size() * sizeof(int) + sizeof(ResizeTap) - 1) / sizeof(ResizeTap));
			memcpy(taps.data() + hd.chainRegOff, table.data(), table.size() * sizeof(int));
		}
	}
	return MCS_OK;
}

}  // namespace mcs
