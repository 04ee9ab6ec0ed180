// lba_guard_driver.cpp — runs the argument checks of mcs_local_bundle_adjustment (csrc/mcs_lba_guard.hip) on small argument structs and prints one line per
// case: name, code, text (tab-separated).  A case calls what the entry point calls, in its order.  No HIP call; tests/test_lba_cpu.py.
#include "mcs_lba.h"

#include <cstdio>
#include <functional>

std::string& mcs_err() { static std::string e; return e; }   // the library's is in mcs_capi.hip
using namespace mcs;

static const mcs_ctx* const CTX = reinterpret_cast<const mcs_ctx*>(0x1000);   // the checks only compare it with null

// valid arguments: 3 keyframes (2 local, 1 free), 2 points of 2 edges, 2 cameras, 3 levels; a case spoils its copy
struct Args {
	std::vector<double> pose = std::vector<double>(18, 0.0);
	std::vector<uint8_t> fixed = {1, 0, 1};
	double pos[6] = {}, Mc[12] = {}, sig[3] = {1.0, 0.7, 0.5};
	int32_t first[3] = {0, 2, 4}, ekf[4] = {0, 1, 1, 2}, ecam[4] = {0, 1, 0, 1};
	mcs_keypoint keys[4] = {};
	uint8_t es[4] = {}, ps[2] = {};
	mcs_ocam ocam[2] = {};
	int nKfs = 3, nLocal = 2, nPoints = 2, nEdges = 4, nr = 2, nlevels = 3;
	mcs_mem_kind kind = MCS_MEM_HOST;
	bool deferred = false;
	const mcs_ctx* ctx = CTX;
	Args() { for (mcs_ocam& o : ocam) { o.p_deg = 5; o.invP_deg = 12; o.width = 64; o.height = 48; } keys[1].octave = 2; }
	int run() {
		const LbaCall q{nKfs, nLocal, pose.data(), fixed.data(), nullptr, nPoints, pos, first, nEdges, ekf, ecam, keys, nullptr, nullptr, Mc, ocam, nr, sig, nlevels,
		                2.0, nullptr, kind, es, ps, nullptr};
		if (int r = guard_lba(ctx, q, deferred)) return r;
		int nFree = 0;
		if (int r = guard_lba_free(fixed.data(), nKfs, &nFree)) return r;
		return kind == MCS_MEM_HOST ? guard_lba_content(q) : MCS_OK;
	}
};

int main() {
	const std::pair<const char*, std::function<void(Args&)>> cases[] = {
		{"valid", [](Args&) {}},
		{"null_ctx", [](Args& a) { a.ctx = nullptr; }},
		{"kind", [](Args& a) { a.kind = (mcs_mem_kind)7; }},
		{"negative", [](Args& a) { a.nPoints = -1; }},
		{"local>kfs", [](Args& a) { a.nLocal = 4; }},
		{"cams_0", [](Args& a) { a.nr = 0; }},
		{"cams_33", [](Args& a) { a.nr = 33; }},
		{"levels_0", [](Args& a) { a.nlevels = 0; }},
		{"kfs_4097", [](Args& a) { a.nKfs = 4097; }},
		{"points", [](Args& a) { a.nPoints = (1 << 20) + 1; }},
		{"edges", [](Args& a) { a.nEdges = (1 << 22) + 1; }},
		{"free_64", [](Args& a) { a.nKfs = 65; a.pose.assign(65 * 6, 0.0); a.fixed.assign(65, 0); a.fixed[64] = 1; }},
		{"free_65", [](Args& a) { a.nKfs = 65; a.pose.assign(65 * 6, 0.0); a.fixed.assign(65, 0); }},
		{"free_65.device", [](Args& a) { a.nKfs = 65; a.pose.assign(65 * 6, 0.0); a.fixed.assign(65, 0); a.kind = MCS_MEM_DEVICE; }},
		{"deferred", [](Args& a) { a.deferred = true; }},
		{"deferred+kf", [](Args& a) { a.deferred = true; a.ekf[0] = 3; }},
		{"first.negative", [](Args& a) { a.first[0] = -1; }},
		{"first.backwards", [](Args& a) { a.first[1] = 3; a.first[2] = 2; }},
		{"first.beyond", [](Args& a) { a.first[2] = 5; }},
		{"first.device", [](Args& a) { a.first[2] = 5; a.kind = MCS_MEM_DEVICE; }},
		{"kf", [](Args& a) { a.ekf[3] = 3; }},
		{"kf.negative", [](Args& a) { a.ekf[0] = -1; }},
		{"kf.device", [](Args& a) { a.ekf[3] = 3; a.kind = MCS_MEM_DEVICE; }},
		{"camera", [](Args& a) { a.ecam[0] = 2; }},
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
