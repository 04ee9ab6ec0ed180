// mcs_window_guard.hip — the argument checks of the grid-window search family (mcs_window.h).  No HIP call in this file.
#include "mcs_window.h"

namespace mcs {

int null_argument() { return fail(MCS_ERR_INVALID, "null argument"); }
static int bad_sizes() { return fail(MCS_ERR_INVALID, "bad sizes"); }
static int bad_frame_sizes() { return fail(MCS_ERR_INVALID, "bad sizes (frame features must be <= 65536)"); }
static int bad_level() { return fail(MCS_ERR_INVALID, "projection level outside [0, nlevels)"); }

// the three checks every search of the family makes between its own size check and whatever follows
static int check_dim(int dim) {
	if (dim != 16 && dim != 32 && dim != 64) return fail(MCS_ERR_INVALID, "dim must be 16, 32 or 64");
	return MCS_OK;
}
static int check_masks_strides(const uint8_t* pmask, int pstride, const mcs_frame_view* f, int dim) {
	if ((pmask == nullptr) != (f->mask == nullptr)) return fail(MCS_ERR_INVALID, "masks must be given for both sides or neither");
	if (pstride < dim || f->stride < dim || (pstride & 3) || (f->stride & 3)) return fail(MCS_ERR_INVALID, "descriptor stride must be >= dim and a multiple of 4");
	return MCS_OK;
}

int guard_image_size(const mcs_ocam& cam) {
	if (cam.width < 1 || cam.height < 1) return fail(MCS_ERR_INVALID, "bad image size");
	return MCS_OK;
}
static int check_rig_cameras(const mcs_rig_view* rig, int nr) {
	for (int k = 0; k < nr; ++k) {
		if (rig->cams[k].invP_deg < 1 || rig->cams[k].invP_deg > MCS_MAX_POLY) return bad_polynomial_degree();
		if (int r = guard_image_size(rig->cams[k])) return r;
		if (rig->mirror_masks && !rig->mirror_masks[k]) return fail(MCS_ERR_INVALID, "null mirror mask");
	}
	return MCS_OK;
}

int guard_search_by_projection(const mcs_ctx* c, const mcs_projection_set* mp, const mcs_frame_view* f, int dim, bool hostKind, const int32_t* match,
                               const int32_t* nmatches) {
	if (!c || !mp || !f || !match || !nmatches) return null_argument();
	if (int r = check_dim(dim)) return r;
	if (mp->n < 0 || f->n < 0 || f->n > 65536 || f->nr_cams < 1 || f->nlevels < 1) return bad_frame_sizes();
	if (int r = check_masks_strides(mp->mask, mp->stride, f, dim)) return r;
	if (hostKind)   // level[] indexes scale_factors on the device
		for (int i = 0; i < mp->n; ++i)
			if (mp->level[i] < 0 || mp->level[i] >= f->nlevels) return bad_level();
	return MCS_OK;
}

int guard_window(const mcs_ctx* c, const mcs_window_probes* pr, const mcs_frame_view* f, mcs_window_rule rule, int dim, int bestMode, int maxDist,
                 const int32_t* match, const int32_t* nmatches) {
	if (bestMode && maxDist < 0) return fail(MCS_ERR_INVALID, "max_dist must be >= 0");
	if (!c || !pr || !f || !match || !nmatches) return null_argument();
	if (rule != MCS_WINDOW_RATIO && rule != MCS_WINDOW_BEST && rule != MCS_WINDOW_INITIALIZE) return fail(MCS_ERR_INVALID, "unknown window rule");
	if (int r = check_dim(dim)) return r;
	if (pr->n < 0 || f->n < 0 || f->n > 65536 || f->nr_cams < 1) return bad_frame_sizes();
	if (int r = check_masks_strides(pr->mask, pr->stride, f, dim)) return r;
	if (rule != MCS_WINDOW_INITIALIZE && bestMode != 1 && !f->assigned) return fail(MCS_ERR_INVALID, "frame->assigned is required");
	return MCS_OK;
}

int guard_world_to_cam(const mcs_ctx* c, const double* MtMcInv, const mcs_ocam* cams, int nrCams, const double* pts3, const int32_t* cam, int n, const double* uv,
                       const uint8_t* flags) {
	if (!c || !MtMcInv || !cams || !pts3 || !cam || !uv || !flags) return null_argument();
	if (nrCams < 1 || n < 0) return bad_sizes();
	return MCS_OK;
}

int guard_rotation_consistency(const mcs_ctx* c, int variant, const float* angleSlot, int strideSlot, const float* anglePartner, int stridePartner,
                               const int32_t* match, int n, int nPartner, const int32_t* removed) {
	if (!c || !angleSlot || !anglePartner || !match || !removed) return null_argument();
	if (variant < 0 || variant > 3 || n < 0 || nPartner < 0 || strideSlot < 4 || stridePartner < 4 || (strideSlot & 3) || (stridePartner & 3))
		return fail(MCS_ERR_INVALID, "bad variant / sizes / strides");
	return MCS_OK;
}

int guard_local_points(const mcs_ctx* c, const LocalCall& q, bool asyncSearch) {
	const mcs_local_points* pts = q.pts; const mcs_rig_view* rig = q.rig; const mcs_track_state* stt = q.stt; const mcs_frame_view* f = q.f;
	const bool search = q.search();
	if (!c || !pts || !rig || !stt || !q.nToMatch) return null_argument();
	if (search && (!q.match || !q.nmatches)) return null_argument();
	if (pts->n < 0 || rig->nr_cams < 1 || rig->nr_cams > 32 || (long long)pts->n * rig->nr_cams > 0x7FFFFFFFll / kProjListK) return bad_sizes();
	if (q.nlevels < 1 || q.nlevels > MCS_MAX_LEVELS) return bad_sizes();
	if (search) {
		if (int r = check_dim(q.dim)) return r;
		if (f->n < 0 || f->n > 65536 || f->nr_cams != rig->nr_cams) return bad_frame_sizes();
		if (int r = check_masks_strides(q.mask, q.stride, f, q.dim)) return r;
		if (asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the frustum test and the search run in order: switch deferred searches off (mcs_ctx_set_async_search)");
	}
	if (pts->n > 0) {
		if (!pts->pos || !pts->normal || !pts->min_dist || !pts->max_dist || !pts->flags || !rig->MtMc_inv || !rig->MtMc || !rig->cams || !q.scales || !q.visibleInc ||
		    !stt->in_view || !stt->proj_x || !stt->proj_y || !stt->level || !stt->view_cos)
			return null_argument();
		if (search && (!q.desc || !f->width || !f->height || (f->n > 0 && (!f->keys || !f->desc || !f->cam || !f->assigned)))) return null_argument();
	}
	return MCS_OK;
}

int guard_local_points_content(const LocalCall& q) {
	const mcs_local_points* pts = q.pts; const mcs_rig_view* rig = q.rig; const mcs_track_state* stt = q.stt;
	const int np = pts->n, nr = rig->nr_cams, nlevels = q.nlevels;
	if (np == 0) return MCS_OK;   // nothing is read of an empty call (the entry point has returned by now)
	if (int r = check_rig_cameras(rig, nr)) return r;
	if (q.search())
		for (int i = 0; i < np; ++i) {
			if ((pts->flags[i] & (MCS_LP_BAD | MCS_LP_SEEN)) != MCS_LP_SEEN) continue;   // the stale slots SearchByProjection reads (bits 0 and 1 alone count)
			for (int k = 0; k < nr; ++k)
				if (stt->in_view[(size_t)i * nr + k] && (stt->level[(size_t)i * nr + k] < 0 || stt->level[(size_t)i * nr + k] >= nlevels)) return bad_level();
		}
	return MCS_OK;
}

int guard_tracked(const mcs_ctx* c, const TrackedCall& q, bool asyncSearch) {
	const mcs_tracked_frame* tf = q.tf; const mcs_point_table* pts = q.pts; const mcs_rig_view* rig = q.rig; const mcs_frame_view* f = q.f;
	const bool project = q.project();
	if (!c || !tf || !pts || !f || !q.matchFeat || !q.nmatches) return null_argument();
	if (int r = check_dim(q.dim)) return r;
	if (tf->n < 0 || tf->n > 65536 || f->n < 0 || f->n > 65536 || pts->n < 0 || f->nr_cams < 1 || f->nr_cams > 32) return bad_frame_sizes();
	if (project && (rig->nr_cams != f->nr_cams || f->nlevels < 1 || f->nlevels > MCS_MAX_LEVELS))
		return fail(MCS_ERR_INVALID, "bad sizes (rig and frame must agree on the cameras)");
	if (int r = check_masks_strides(tf->mask, tf->stride, f, q.dim)) return r;
	if (asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the probes and the search run in order: switch deferred searches off (mcs_ctx_set_async_search)");
	if (tf->n > 0 && f->n > 0) {
		if (!tf->keys || !tf->desc || !tf->cam || !tf->points || !f->keys || !f->desc || !f->cam || !f->width || !f->height || (pts->n > 0 && (!pts->pos || !pts->flags)))
			return null_argument();
		if (project && (!rig->MtMc_inv || !rig->cams || !f->scale_factors || !f->assigned)) return null_argument();
	}
	return MCS_OK;
}

int guard_tracked_content(const TrackedCall& q) {
	const mcs_tracked_frame* tf = q.tf; const mcs_point_table* pts = q.pts; const mcs_rig_view* rig = q.rig; const mcs_frame_view* f = q.f;
	const bool project = q.project();
	const int nr = f->nr_cams;
	if (tf->n == 0 || f->n == 0) return MCS_OK;   // nothing is read of an empty call (the entry point has returned by now)
	if (project)
		if (int r = check_rig_cameras(rig, nr)) return r;
	for (int i = 0; i < tf->n; ++i) {
		if (tf->points[i] < 0) continue;   // NULL: nothing of this feature is read
		if (tf->points[i] >= pts->n) return fail(MCS_ERR_INVALID, "map point id outside [0, points->n)");
		if (tf->cam[i] < 0 || tf->cam[i] >= nr) return fail(MCS_ERR_INVALID, "camera index outside [0, nr_cams)");
		if (project && (tf->keys[i].octave < 0 || tf->keys[i].octave >= f->nlevels)) return fail(MCS_ERR_INVALID, "key octave outside [0, nlevels)");
	}
	return MCS_OK;
}

}  // namespace mcs
