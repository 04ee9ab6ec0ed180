// mcs_essgraph.h — what the pieces of mcs_optimize_essential_graph share: the call's arguments and its argument checks (mcs_essgraph_guard.hip: host logic
// only, no HIP call).  The kernels and the host loop are mcs_essgraph.hip.
#pragma once
#include "mcs_host.h"

namespace mcs {

constexpr int kEgMaxFree = 512;        // free Sim3 vertices: the system is at most 3584 x 3584 (103 MB)
constexpr int kEgMaxKfs = 4096;
constexpr int kEgMaxEdges = 1 << 17;   // 929 bytes of scratch per edge (both Jacobians, the residual, the measurement, the lists): 122 MB at the limit
constexpr int kEgMaxPoints = 1 << 22;
constexpr int kEgPanel = 32;           // the panel width of the blocked LDL^T: with the problem it decides the order of every inner sum

struct EgCall {
	int nKfs; const double* Scw; const double* Snc; const uint8_t* hasNc; const uint8_t* kfFixed; int nEdges; const int32_t* edgeI; const int32_t* edgeJ;
	const uint8_t* edgeKind; int nPoints; double* pos; const int32_t* ptRef; mcs_mem_kind kind; double* ScwOut; double* pose; double* kfT; mcs_eg_diag* diag;
};
// MCS_OK, or the refusal's code with its text left for mcs_last_error(); `c` is only compared with null.  asyncSearch: deferred searches are on.
int guard_eg(const mcs_ctx* c, const EgCall& q, bool asyncSearch);
// the free vertices among kfFixed[nKfs] (a HOST copy for either kind) -> MCS_OK and *nFree, or MCS_ERR_CAPACITY above kEgMaxFree
int guard_eg_free(const uint8_t* kfFixedHost, int nKfs, int* nFree);
// the scan of a host-kind call's contents: what the kernels index with (device kind: such an edge contributes nothing, such a point stays untouched)
int guard_eg_content(const EgCall& q);

}  // namespace mcs
