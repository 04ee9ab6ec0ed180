// mcs_poseopt_guard.hip — the argument checks of mcs_pose_optimization (mcs_poseopt.h).  No HIP call in this file.
#include "mcs_poseopt.h"

namespace mcs {

static int pose_null() { return fail(MCS_ERR_INVALID, "null argument"); }

int guard_pose(const mcs_ctx* c, const PoseCall& q, bool asyncSearch) {
	if (q.nproblems < 0) return fail(MCS_ERR_INVALID, "bad sizes (nproblems must be >= 0)");
	if (q.nproblems == 0) return MCS_OK;
	if (!c || !q.frames || !q.pts || !q.McMin || !q.cams || !q.invSigma2 || !q.huber || !q.poseMin || !q.outlier || !q.nInliers || !q.share) return pose_null();
	if (q.kind != MCS_MEM_HOST && q.kind != MCS_MEM_DEVICE) return fail(MCS_ERR_INVALID, "unknown memory kind");
	if (q.nrCams < 1 || q.nrCams > 32 || q.nlevels < 1 || q.nlevels > MCS_MAX_LEVELS || q.pts->n < 0) return fail(MCS_ERR_INVALID, "bad sizes");
	if (asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the optimisation runs in the order of the context's stream: switch deferred searches off (mcs_ctx_set_async_search)");
	if (q.pts->n > 0 && !q.pts->pos) return pose_null();
	for (int p = 0; p < q.nproblems; ++p) {
		const mcs_pose_frame& f = q.frames[p];
		if (f.n < 0 || f.n > 65536) return fail(MCS_ERR_INVALID, "bad sizes (frame features must be <= 65536)");
		if (f.n > 0 && (!f.keys || !f.cam || !f.points || !q.outlier[p])) return pose_null();
	}
	return MCS_OK;
}

int guard_pose_content(const PoseCall& q) {
	for (int k = 0; k < q.nrCams; ++k)
		if (q.cams[k].invP_deg < 1 || q.cams[k].invP_deg > MCS_MAX_POLY) return bad_polynomial_degree();
	for (int p = 0; p < q.nproblems; ++p) {
		const mcs_pose_frame& f = q.frames[p];
		for (int i = 0; i < f.n; ++i) {
			if (f.points[i] < 0) continue;   // NULL: nothing of this feature is read
			if (f.points[i] >= q.pts->n) return fail(MCS_ERR_INVALID, "map point id outside [0, points->n)");
			if (f.cam[i] < 0 || f.cam[i] >= q.nrCams) return fail(MCS_ERR_INVALID, "camera index outside [0, nr_cams)");
			if (f.keys[i].octave < 0 || f.keys[i].octave >= q.nlevels) return fail(MCS_ERR_INVALID, "key octave outside [0, nlevels)");
		}
	}
	return MCS_OK;
}

}  // namespace mcs
