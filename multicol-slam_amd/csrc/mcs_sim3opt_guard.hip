// mcs_sim3opt_guard.hip — the argument checks of mcs_sim3_optimize (mcs_sim3opt.h).  No HIP call in this file.
#include "mcs_sim3opt.h"

namespace mcs {

static int sim3opt_null() { return fail(MCS_ERR_INVALID, "null argument"); }

int guard_sim3opt(const mcs_ctx* c, const Sim3OptCall& q, bool asyncSearch) {
	if (q.nproblems < 0) return fail(MCS_ERR_INVALID, "bad sizes (nproblems must be >= 0)");
	if (q.nproblems == 0) return MCS_OK;
	if (!c || !q.probs || !q.Mc || !q.cams || !q.MtInv || !q.stdSim || !q.R12 || !q.t12 || !q.s12 || !q.S12 || !q.keep || !q.nInliers) return sim3opt_null();
	if (q.kind != MCS_MEM_HOST && q.kind != MCS_MEM_DEVICE) return fail(MCS_ERR_INVALID, "unknown memory kind");
	if (q.nrCams < 1 || q.nrCams > 32) return fail(MCS_ERR_INVALID, "bad sizes");
	if (asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the optimisation runs in the order of the context's stream: switch deferred searches off (mcs_ctx_set_async_search)");
	for (int p = 0; p < q.nproblems; ++p) {
		const mcs_sim3opt_problem& f = q.probs[p];
		if (f.n < 0 || f.n > 65536) return fail(MCS_ERR_INVALID, "bad sizes (correspondences must be <= 65536)");
		if (f.n > 0 && (!f.Xw || !f.cam || !f.obs || !f.w || !q.keep[p])) return sim3opt_null();
	}
	return MCS_OK;
}

int guard_sim3opt_content(const Sim3OptCall& q) {
	for (int k = 0; k < q.nrCams; ++k)
		if (q.cams[k].invP_deg < 1 || q.cams[k].invP_deg > MCS_MAX_POLY) return bad_polynomial_degree();
	for (int p = 0; p < q.nproblems; ++p) {
		const mcs_sim3opt_problem& f = q.probs[p];
		for (int i = 0; i < 2 * f.n; ++i)
			if (f.cam[i] < 0 || f.cam[i] >= q.nrCams) return fail(MCS_ERR_INVALID, "camera index outside [0, nr_cams)");
	}
	return MCS_OK;
}

}  // namespace mcs
