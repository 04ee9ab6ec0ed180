// essgraph_guard_driver.cpp — runs the argument checks of mcs_optimize_essential_graph (csrc/mcs_essgraph_guard.hip) on small argument structs and prints one
// line per case: name, code, text (tab-separated).  A case calls what the entry point calls, in its order.  No HIP call; tests/test_essgraph_capi_cpu.py.
#include "mcs_essgraph.h"

#include <cstdio>
#include <functional>

std::string& mcs_err() { static std::string e; return e; }   // the library's is in mcs_capi.hip
using namespace mcs;

static const mcs_ctx* const CTX = reinterpret_cast<const mcs_ctx*>(0x1000);   // the checks only compare it with null

// valid arguments: 3 keyframes (1 fixed), 3 edges, 2 points; a case spoils its copy
struct Args {
	std::vector<double> S = std::vector<double>(24, 0.0), out = std::vector<double>(24, 0.0), pose = std::vector<double>(48, 0.0);
	std::vector<uint8_t> nc = {0, 0, 1}, fixed = {1, 0, 0};
	int32_t ei[3] = {2, 1, 2}, ej[3] = {0, 0, 1}, ref[2] = {1, -1};
	uint8_t kind[3] = {0, 1, 1};
	double pos[6] = {};
	int nKfs = 3, nEdges = 3, nPoints = 2;
	mcs_mem_kind mem = MCS_MEM_HOST;
	bool deferred = false, noOut = false;
	const mcs_ctx* ctx = CTX;
	void grow(int n, int nFixed) { nKfs = n; S.assign(8 * n, 0.0); out.assign(8 * n, 0.0); pose.assign(16 * n, 0.0); nc.assign(n, 0); fixed.assign(n, 0); for (int k = 0; k < nFixed; ++k) fixed[k] = 1; }
	int run() {
		const EgCall q{nKfs, S.data(), S.data(), nc.data(), fixed.data(), nEdges, ei, ej, kind, nPoints, pos, ref, mem, noOut ? nullptr : out.data(), pose.data(), nullptr, nullptr};
		if (int r = guard_eg(ctx, q, deferred)) return r;
		int nFree = 0;
		if (int r = guard_eg_free(fixed.data(), nKfs, &nFree)) return r;
		return mem == MCS_MEM_HOST ? guard_eg_content(q) : MCS_OK;
	}
};

int main() {
	const std::pair<const char*, std::function<void(Args&)>> cases[] = {
		{"valid", [](Args&) {}},
		{"null_ctx", [](Args& a) { a.ctx = nullptr; }},
		{"kind", [](Args& a) { a.mem = (mcs_mem_kind)7; }},
		{"negative", [](Args& a) { a.nEdges = -1; }},
		{"null_out", [](Args& a) { a.noOut = true; }},
		{"kfs_4097", [](Args& a) { a.grow(4097, 4000); }},
		{"edges", [](Args& a) { a.nEdges = (1 << 17) + 1; }},
		{"points", [](Args& a) { a.nPoints = (1 << 22) + 1; }},
		{"free_512", [](Args& a) { a.grow(513, 1); }},
		{"free_513", [](Args& a) { a.grow(513, 0); }},
		{"free_513.device", [](Args& a) { a.grow(513, 0); a.mem = MCS_MEM_DEVICE; }},
		{"deferred", [](Args& a) { a.deferred = true; }},
		{"edge.beyond", [](Args& a) { a.ei[1] = 3; }},
		{"edge.negative", [](Args& a) { a.ej[2] = -1; }},
		{"edge.self", [](Args& a) { a.ej[0] = 2; }},
		{"edge.device", [](Args& a) { a.ei[1] = 3; a.mem = MCS_MEM_DEVICE; }},
		{"ref.beyond", [](Args& a) { a.ref[0] = 3; }},
		{"ref.minus2", [](Args& a) { a.ref[1] = -2; }},
		{"ref.device", [](Args& a) { a.ref[0] = 3; a.mem = MCS_MEM_DEVICE; }},
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
