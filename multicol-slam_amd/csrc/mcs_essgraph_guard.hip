// mcs_essgraph_guard.hip — the argument checks of mcs_optimize_essential_graph (mcs_essgraph.h).  No HIP call in this file.
#include "mcs_essgraph.h"

namespace mcs {

static int eg_null() { return fail(MCS_ERR_INVALID, "null argument"); }

int guard_eg(const mcs_ctx* c, const EgCall& q, bool asyncSearch) {
	if (!c) return eg_null();
	if (q.kind != MCS_MEM_HOST && q.kind != MCS_MEM_DEVICE) return fail(MCS_ERR_INVALID, "unknown memory kind");
	if (q.nKfs < 0 || q.nEdges < 0 || q.nPoints < 0) return fail(MCS_ERR_INVALID, "bad sizes");
	if (q.nKfs > kEgMaxKfs) return fail(MCS_ERR_CAPACITY, "more than 4096 keyframes");
	if (q.nEdges > kEgMaxEdges) return fail(MCS_ERR_CAPACITY, "more than 2^17 edges");
	if (q.nPoints > kEgMaxPoints) return fail(MCS_ERR_CAPACITY, "more than 2^22 points");
	if (asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the optimisation runs in the order of the context's stream: switch deferred searches off (mcs_ctx_set_async_search)");
	if (q.nKfs > 0 && (!q.Scw || !q.Snc || !q.hasNc || !q.kfFixed || !q.ScwOut || !q.pose)) return eg_null();
	if (q.nEdges > 0 && (!q.edgeI || !q.edgeJ || !q.edgeKind)) return eg_null();
	if (q.nPoints > 0 && (!q.pos || !q.ptRef)) return eg_null();
	return MCS_OK;
}

int guard_eg_free(const uint8_t* kfFixedHost, int nKfs, int* nFree) {
	int n = 0;
	for (int k = 0; k < nKfs; ++k) n += kfFixedHost[k] ? 0 : 1;
	*nFree = n;
	if (n > kEgMaxFree) return fail(MCS_ERR_CAPACITY, "more than 512 free keyframes (the system is at most 3584 x 3584)");
	return MCS_OK;
}

int guard_eg_content(const EgCall& q) {
	for (int e = 0; e < q.nEdges; ++e) {
		if (q.edgeI[e] < 0 || q.edgeI[e] >= q.nKfs || q.edgeJ[e] < 0 || q.edgeJ[e] >= q.nKfs) return fail(MCS_ERR_INVALID, "edge vertex outside [0, n_kfs)");
		if (q.edgeI[e] == q.edgeJ[e]) return fail(MCS_ERR_INVALID, "an edge joins a vertex with itself");
	}
	for (int p = 0; p < q.nPoints; ++p)
		if (q.ptRef[p] < -1 || q.ptRef[p] >= q.nKfs) return fail(MCS_ERR_INVALID, "pt_ref outside [-1, n_kfs)");
	return MCS_OK;
}

}  // namespace mcs
