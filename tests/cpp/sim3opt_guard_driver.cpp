// sim3opt_guard_driver.cpp — runs the argument checks of mcs_sim3_optimize (csrc/mcs_sim3opt_guard.hip) on small argument structs and prints one line per
// case: name, code, text (tab-separated).  A case calls what the entry point calls, in its order.  No HIP call; tests/test_sim3opt_cpu.py.  A stand-alone
// program: it may also be built with -fsanitize=address,undefined and run on the CPU.
#include "mcs_sim3opt.h"

#include <cstdio>
#include <functional>

std::string& mcs_err() { static std::string e; return e; }   // the library's is in mcs_capi.hip
using namespace mcs;

static const mcs_ctx* const CTX = reinterpret_cast<const mcs_ctx*>(0x1000);   // the checks only compare it with null

// valid arguments: 2 problems of 3 and 0 correspondences, 2 cameras; a case spoils its copy
struct Args {
	double Xw[18] = {}, obs[12] = {}, w[6] = {1, 1, 1, 1, 1, 1}, Mc[32] = {}, Mt[64] = {}, stdSim[2] = {4.0, 4.0}, R[18] = {}, t[6] = {}, s[2] = {1.0, 1.0}, S12[16] = {};
	int32_t cam[6] = {0, 1, 1, 0, 0, 0}, nin[2] = {};
	uint8_t keep0[3] = {};
	uint8_t* keeps[2] = {keep0, nullptr};
	mcs_ocam ocam[2] = {};
	mcs_sim3opt_problem probs[2] = {{Xw, cam, obs, w, 3}, {nullptr, nullptr, nullptr, nullptr, 0}};
	int nproblems = 2, nr = 2;
	mcs_mem_kind kind = MCS_MEM_HOST;
	bool deferred = false;
	const mcs_ctx* ctx = CTX;
	double* S12p = S12;
	const double* Mtp = Mt;
	Args() { for (mcs_ocam& o : ocam) { o.p_deg = 5; o.invP_deg = 12; o.width = 64; o.height = 48; } }
	int run() {
		const Sim3OptCall q{nproblems, probs, Mc, ocam, nr, Mtp, stdSim, R, t, s, kind, S12p, nullptr, keeps, nin, nullptr};
		if (int r = guard_sim3opt(ctx, q, deferred)) return r;
		if (nproblems == 0) return MCS_OK;
		return kind == MCS_MEM_HOST ? guard_sim3opt_content(q) : MCS_OK;
	}
};

int main() {
	const std::pair<const char*, std::function<void(Args&)>> cases[] = {
		{"valid", [](Args&) {}},
		{"empty", [](Args& a) { a.nproblems = 0; a.ctx = nullptr; }},
		{"negative", [](Args& a) { a.nproblems = -1; }},
		{"null_ctx", [](Args& a) { a.ctx = nullptr; }},
		{"null_keep", [](Args& a) { a.keeps[0] = nullptr; }},
		{"null_keep_of_empty", [](Args& a) { a.keeps[1] = nullptr; }},
		{"null_Xw", [](Args& a) { a.probs[0].Xw = nullptr; }},
		{"null_w", [](Args& a) { a.probs[0].w = nullptr; }},
		{"null_S12", [](Args& a) { a.S12p = nullptr; }},
		{"null_Mt", [](Args& a) { a.Mtp = nullptr; }},
		{"cams_0", [](Args& a) { a.nr = 0; }},
		{"cams_33", [](Args& a) { a.nr = 33; }},
		{"correspondences", [](Args& a) { a.probs[0].n = 65537; }},
		{"correspondences.negative", [](Args& a) { a.probs[1].n = -1; }},
		{"deferred", [](Args& a) { a.deferred = true; }},
		{"deferred+camera", [](Args& a) { a.deferred = true; a.cam[0] = 2; }},
		{"camera", [](Args& a) { a.cam[0] = 2; }},
		{"camera.second", [](Args& a) { a.cam[5] = 2; }},
		{"camera.negative", [](Args& a) { a.cam[3] = -1; }},
		{"camera.device", [](Args& a) { a.cam[0] = 2; a.kind = MCS_MEM_DEVICE; }},
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
