// mcs_sim3opt.h — what the pieces of mcs_sim3_optimize share: the call's arguments, its argument checks (mcs_sim3opt_guard.hip: host logic only, no HIP
// call; tests/test_sim3opt_cpu.py runs it alone) and the kernel's launcher (mcs_sim3opt.hip).
#pragma once
#include "mcs_host.h"

namespace mcs {

struct Sim3OptCall {
	int nproblems; const mcs_sim3opt_problem* probs; const double* Mc; const mcs_ocam* cams; int nrCams; const double* MtInv; const double* stdSim;
	const double* R12; const double* t12; const double* s12; mcs_mem_kind kind;
	double* S12; double* R12out; uint8_t* const* keep; int32_t* nInliers; mcs_sim3opt_diag* diag;
};
// MCS_OK, or the refusal's code with its text left for mcs_last_error(); `c` is only compared with null.  asyncSearch: deferred searches are on.
// nproblems == 0 passes (the entry point returns before it reads anything else).
int guard_sim3opt(const mcs_ctx* c, const Sim3OptCall& q, bool asyncSearch);
// the scan of a host-kind call's contents: what the kernel indexes with (device kind: such a correspondence gives no edge pair)
int guard_sim3opt_content(const Sim3OptCall& q);

// The kernel takes the per-problem pointers BY VALUE, kSim3OptBatch problems per launch: a device-kind call uploads no table and so never waits for the stream.
constexpr int kSim3OptBatch = 64;
constexpr int kSim3OptThreads = 256;
struct Sim3OptChunk {
	const double* Xw[kSim3OptBatch]; const int* cam[kSim3OptBatch]; const double* obs[kSim3OptBatch]; const double* w[kSim3OptBatch];
	uint8_t* keep[kSim3OptBatch]; int n[kSim3OptBatch];
};
struct Sim3OptArgs {
	const double* Mc; const mcs_ocam* cams; int nrCams; const double* MtInv; const double* stdSim; const double* R12; const double* t12; const double* s12;
	double* S12; double* R12out; int* nInliers; mcs_sim3opt_diag* diag;   // indexed by the problem's place in the whole batch
};
void launch_sim3opt(const Sim3OptArgs& a, const Sim3OptChunk& ch, int first, int count, hipStream_t s);   // problems [first, first + count), count <= kSim3OptBatch

}  // namespace mcs
