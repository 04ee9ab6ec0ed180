// mcs_lba.h — what the pieces of mcs_local_bundle_adjustment share: the call's arguments and its argument checks (mcs_lba_guard.hip: host logic only, no HIP
// call; tests/test_lba_cpu.py runs it alone).  The kernels and the host loop are mcs_lba.hip.
#pragma once
#include "mcs_host.h"

namespace mcs {

constexpr int kLbaMaxFree = 64;        // free pose vertices: the reduced system is at most 384 x 384
constexpr int kLbaMaxKfs = 4096;
constexpr int kLbaMaxPoints = 1 << 20;
constexpr int kLbaMaxEdges = 1 << 22;

struct LbaCall {
	int nKfs, nLocal; double* kfPoseMin; const uint8_t* kfFixed; double* kfT; int nPoints; double* pos; const int32_t* ptFirst; int nEdges;
	const int32_t* edgeKf; const int32_t* edgeCam; const mcs_keypoint* edgeKey; const int32_t* ptTotalObs; const int32_t* ptBadObs;
	const double* McMin; const mcs_ocam* cams; int nrCams; const double* invSigma2; int nlevels; double stdRecon; int* stopFlag; mcs_mem_kind kind;
	uint8_t* edgeState; uint8_t* ptState; mcs_lba_diag* diag;
};
// MCS_OK, or the refusal's code with its text left for mcs_last_error(); `c` is only compared with null.  asyncSearch: deferred searches are on.
int guard_lba(const mcs_ctx* c, const LbaCall& q, bool asyncSearch);
// the free pose vertices among kfFixed[nKfs] (a HOST copy for either kind) -> MCS_OK and *nFree, or MCS_ERR_CAPACITY above kLbaMaxFree
int guard_lba_free(const uint8_t* kfFixedHost, int nKfs, int* nFree);
// the scan of a host-kind call's contents: what the kernels index with (device kind: such an edge contributes nothing)
int guard_lba_content(const LbaCall& q);

}  // namespace mcs
