// poseopt_guard_driver.cpp — runs the argument checks of mcs_pose_optimization (csrc/mcs_poseopt_guard.hip) on small argument structs and prints one line per
// case: name, code, text (tab-separated).  A case calls what the entry point calls, in its order.  No HIP call; tests/test_poseopt_cpu.py.
#include "mcs_poseopt.h"

#include <cstdio>
#include <functional>

std::string& mcs_err() { static std::string e; return e; }   // the library's is in mcs_capi.hip
using namespace mcs;

static const mcs_ctx* const CTX = reinterpret_cast<const mcs_ctx*>(0x1000);   // the checks only compare it with null

// valid arguments: 2 problems of 3 and 0 features, 2 cameras, 3 levels, 4 map points; a case spoils its copy
struct Args {
	mcs_keypoint keys[3] = {};
	int32_t cam[3] = {0, 1, 0}, points[3] = {0, -1, 3}, nin[2] = {};
	double pos[12] = {}, Mc[12] = {}, sig[3] = {1.0, 0.7, 0.5}, hub[2] = {1.0, 1.0}, pose[12] = {}, share[2] = {};
	uint8_t out0[3] = {};
	uint8_t* outs[2] = {out0, nullptr};
	mcs_ocam ocam[2] = {};
	mcs_pose_frame frames[2] = {{keys, cam, points, 3}, {nullptr, nullptr, nullptr, 0}};
	mcs_point_table tab{pos, nullptr, 4};
	int nproblems = 2, nr = 2, nlevels = 3;
	mcs_mem_kind kind = MCS_MEM_HOST;
	bool deferred = false;
	const mcs_ctx* ctx = CTX;
	Args() { for (mcs_ocam& o : ocam) { o.p_deg = 5; o.invP_deg = 12; o.width = 64; o.height = 48; } keys[1].octave = 2; }
	int run() {
		const PoseCall q{nproblems, frames, &tab, Mc, ocam, nr, sig, nlevels, hub, kind, pose, nullptr, nullptr, outs, nin, share, nullptr};
		if (int r = guard_pose(ctx, q, deferred)) return r;
		if (nproblems == 0) return MCS_OK;
		return kind == MCS_MEM_HOST ? guard_pose_content(q) : MCS_OK;
	}
};

int main() {
	const std::pair<const char*, std::function<void(Args&)>> cases[] = {
		{"valid", [](Args&) {}},
		{"empty", [](Args& a) { a.nproblems = 0; a.ctx = nullptr; }},
		{"negative", [](Args& a) { a.nproblems = -1; }},
		{"null_ctx", [](Args& a) { a.ctx = nullptr; }},
		{"null_outlier", [](Args& a) { a.outs[0] = nullptr; }},
		{"null_keys", [](Args& a) { a.frames[0].keys = nullptr; }},
		{"null_pos", [](Args& a) { a.tab.pos = nullptr; }},
		{"cams_0", [](Args& a) { a.nr = 0; }},
		{"cams_33", [](Args& a) { a.nr = 33; }},
		{"levels_0", [](Args& a) { a.nlevels = 0; }},
		{"features", [](Args& a) { a.frames[0].n = 65537; }},
		{"deferred", [](Args& a) { a.deferred = true; }},
		{"deferred+point", [](Args& a) { a.deferred = true; a.points[0] = 4; }},
		{"point", [](Args& a) { a.points[2] = 4; }},
		{"point.device", [](Args& a) { a.points[2] = 4; a.kind = MCS_MEM_DEVICE; }},
		{"camera", [](Args& a) { a.cam[0] = 2; }},
		{"camera.negative", [](Args& a) { a.cam[2] = -1; }},
		{"camera.null_point", [](Args& a) { a.cam[1] = 7; }},
		{"octave", [](Args& a) { a.keys[0].octave = 3; }},
		{"octave.device", [](Args& a) { a.keys[0].octave = -1; a.kind = MCS_MEM_DEVICE; }},
		{"polynomial", [](Args& a) { a.ocam[1].invP_deg = 17; }},
	};
	for (const auto& c : cases) {
		Args a;
		c.second(a);
		mcs_err().clear();
		const int rc = a.run();
		std::printf("%s\t%d\t%s\n", c.first, rc, rc ? mcs_err().c_str() : "");
	}
	return 0;
}
