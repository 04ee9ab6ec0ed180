// mcs_lba_guard.hip — the argument checks of mcs_local_bundle_adjustment (mcs_lba.h).  No HIP call in this file.
#include "mcs_lba.h"

namespace mcs {

static int lba_null() { return fail(MCS_ERR_INVALID, "null argument"); }

int guard_lba(const mcs_ctx* c, const LbaCall& q, bool asyncSearch) {
	if (!c) return lba_null();
	if (q.kind != MCS_MEM_HOST && q.kind != MCS_MEM_DEVICE) return fail(MCS_ERR_INVALID, "unknown memory kind");
	if (q.nKfs < 0 || q.nLocal < 0 || q.nLocal > q.nKfs || q.nPoints < 0 || q.nEdges < 0 || q.nrCams < 1 || q.nlevels < 1 || q.nlevels > MCS_MAX_LEVELS)
		return fail(MCS_ERR_INVALID, "bad sizes");
	if (q.nrCams > 32) return fail(MCS_ERR_CAPACITY, "more than 32 cameras");
	if (q.nKfs > kLbaMaxKfs) return fail(MCS_ERR_CAPACITY, "more than 4096 keyframes");
	if (q.nPoints > kLbaMaxPoints) return fail(MCS_ERR_CAPACITY, "more than 2^20 points");
	if (q.nEdges > kLbaMaxEdges) return fail(MCS_ERR_CAPACITY, "more than 2^22 edges");
	if (asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the optimisation runs in the order of the context's stream: switch deferred searches off (mcs_ctx_set_async_search)");
	if (!q.McMin || !q.cams || !q.invSigma2 || !q.ptFirst || !q.edgeState || !q.ptState) return lba_null();
	if (q.nKfs > 0 && (!q.kfPoseMin || !q.kfFixed)) return lba_null();
	if (q.nPoints > 0 && !q.pos) return lba_null();
	if (q.nEdges > 0 && (!q.edgeKf || !q.edgeCam || !q.edgeKey)) return lba_null();
	return MCS_OK;
}

int guard_lba_free(const uint8_t* kfFixedHost, int nKfs, int* nFree) {
	int n = 0;
	for (int k = 0; k < nKfs; ++k) n += kfFixedHost[k] ? 0 : 1;
	*nFree = n;
	if (n > kLbaMaxFree) return fail(MCS_ERR_CAPACITY, "more than 64 free keyframes (the reduced system is at most 384 x 384)");
	return MCS_OK;
}

int guard_lba_content(const LbaCall& q) {
	for (int k = 0; k < q.nrCams; ++k)
		if (q.cams[k].invP_deg < 1 || q.cams[k].invP_deg > MCS_MAX_POLY) return bad_polynomial_degree();
	if (q.ptFirst[0] < 0) return fail(MCS_ERR_INVALID, "pt_first is not monotone within [0, n_edges]");
	for (int p = 0; p < q.nPoints; ++p)
		if (q.ptFirst[p + 1] < q.ptFirst[p] || q.ptFirst[p + 1] > q.nEdges) return fail(MCS_ERR_INVALID, "pt_first is not monotone within [0, n_edges]");
	for (int e = 0; e < q.nEdges; ++e) {
		if (q.edgeKf[e] < 0 || q.edgeKf[e] >= q.nKfs) return fail(MCS_ERR_INVALID, "keyframe index outside [0, n_kfs)");
		if (q.edgeCam[e] < 0 || q.edgeCam[e] >= q.nrCams) return fail(MCS_ERR_INVALID, "camera index outside [0, nr_cams)");
		if (q.edgeKey[e].octave < 0 || q.edgeKey[e].octave >= q.nlevels) return fail(MCS_ERR_INVALID, "key octave outside [0, nlevels)");
	}
	return MCS_OK;
}

}  // namespace mcs
