// mcs_capi_window.hip — C ABI of the grid-window matchers (SearchByProjection(F, mapPoints) and the explicit-window rules) and of the projection they
// consume (include/mcs_c.h: mcs_search_by_projection, mcs_window_match, mcs_world_to_cam), and of the search step of TrackLocalMap that chains the two
// (mcs_frustum, mcs_search_local_points).  Kernels: mcs_project.hip, mcs_frustum.hip.
#include "mcs_host.h"
#include <algorithm>
#include <cstring>
#include <vector>

using namespace mcs;

namespace mcs {
void launch_window_best(const ProjArgs& a, bool skipTaken, int* outDist, hipStream_t s);
void launch_rotation_consistency(int variant, const float* angleSlot, int strideSlot, const float* anglePartner, int stridePartner, const int* accepted, int* match,
                                 int n, int swapped, int* removedOut, hipStream_t s);
}

// What the projection search and the window matchers share: the candidate lists, the probes' camera / descriptor / mask, the frame's arrays and the outputs.
// The scratch makes every call claim the context's block, so a device-kind call ends with a stream synchronisation too (these rows are not bench paths).
static void stage_probes_frame(Staging& st, ProjArgs& a, const int32_t* pcam, const uint8_t* pdesc, const uint8_t* pmask, const mcs_frame_view* f, int32_t* match,
                               int32_t* nmatches) {
	const size_t np = a.nproj, nf = f->n, nc = f->nr_cams;
	st.scratch(&a.lists, np * kProjListK * 8); st.scratch(&a.counts, np * 4);
	st.in(&a.pcam, pcam, np * 4); st.in(&a.pdesc, pdesc, np * a.pstride); st.in(&a.pmask, pmask, np * a.pstride);
	st.in(&a.keys, f->keys, nf * sizeof(mcs_keypoint)); st.in(&a.fdesc, f->desc, nf * f->stride); st.in(&a.fmask, f->mask, nf * f->stride); st.in(&a.fcam, f->cam, nf * 4);
	st.in(&a.width, f->width, nc * 4); st.in(&a.height, f->height, nc * 4);
	st.inout(&a.assigned, f->assigned, nf);
	st.out(&a.match, match, np * 4); st.out(&a.nmatches, nmatches, 4);
}

int mcs_search_by_projection(mcs_ctx* c, const mcs_projection_set* mp, const mcs_frame_view* f, double th, double nnratio, int dim, mcs_mem_kind kind,
                             int32_t* match, int32_t* nmatches) {
	if (!c || !mp || !f || !match || !nmatches) return fail(MCS_ERR_INVALID, "null argument");
	if (dim != 16 && dim != 32 && dim != 64) return fail(MCS_ERR_INVALID, "dim must be 16, 32 or 64");
	if (mp->n < 0 || f->n < 0 || f->n > 65536 || f->nr_cams < 1 || f->nlevels < 1) return fail(MCS_ERR_INVALID, "bad sizes (frame features must be <= 65536)");
	if ((mp->mask == nullptr) != (f->mask == nullptr)) return fail(MCS_ERR_INVALID, "masks must be given for both sides or neither");
	if (mp->stride < dim || f->stride < dim || (mp->stride & 3) || (f->stride & 3)) return fail(MCS_ERR_INVALID, "descriptor stride must be >= dim and a multiple of 4");
	if (kind == MCS_MEM_HOST)   // level[] indexes scale_factors on the device
		for (int i = 0; i < mp->n; ++i)
			if (mp->level[i] < 0 || mp->level[i] >= f->nlevels) return fail(MCS_ERR_INVALID, "projection level outside [0, nlevels)");
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (int r = ctx_join_greedy(c, s)) return r;   // the frame's arrays may come from a search whose greedy pass runs on the side stream
	ProjArgs a{};
	a.nproj = mp->n; a.pstride = mp->stride; a.nfeat = f->n; a.fstride = f->stride; a.nrCams = f->nr_cams;
	a.th = th; a.ratio = nnratio; a.dim = dim; a.rule = 0; a.cap = kProjListK;
	a.thHigh = mp->mask ? (int)floor(1.5 * dim) : 3 * dim;   // TH_HIGH_ (src/cORBmatcher.cpp:46-65)
	const size_t np = mp->n;
	Staging st(c, kind == MCS_MEM_HOST);
	stage_probes_frame(st, a, mp->cam, mp->desc, mp->mask, f, match, nmatches);
	st.in(&a.px, mp->proj_x, np * 8); st.in(&a.py, mp->proj_y, np * 8); st.in(&a.vcos, mp->view_cos, np * 8); st.in(&a.level, mp->level, np * 4);
	st.in(&a.scales, f->scale_factors, (size_t)f->nlevels * 8);
	if (int r = st.commit()) return r;
	if (mp->n > 0) launch_projection(a, s);
	else HIPCHK(hipMemsetAsync(a.nmatches, 0, 4, s));
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

// bestMode 0: mcs_window_match (rule decides); 1: independent best-in-window; 2: best-in-window skipping taken features.  maxDist replaces TH_HIGH
// for bestMode != 0; dist (optional) receives the best distance per probe.
static int window_common(mcs_ctx* c, const mcs_window_probes* pr, const mcs_frame_view* f, mcs_window_rule rule, double nnratio, int dim, mcs_mem_kind kind,
                         int32_t* match, int32_t* nmatches, int bestMode, int maxDist, int32_t* dist) {
	if (!c || !pr || !f || !match || !nmatches) return fail(MCS_ERR_INVALID, "null argument");
	if (rule != MCS_WINDOW_RATIO && rule != MCS_WINDOW_BEST && rule != MCS_WINDOW_INITIALIZE) return fail(MCS_ERR_INVALID, "unknown window rule");
	if (dim != 16 && dim != 32 && dim != 64) return fail(MCS_ERR_INVALID, "dim must be 16, 32 or 64");
	if (pr->n < 0 || f->n < 0 || f->n > 65536 || f->nr_cams < 1) return fail(MCS_ERR_INVALID, "bad sizes (frame features must be <= 65536)");
	if ((pr->mask == nullptr) != (f->mask == nullptr)) return fail(MCS_ERR_INVALID, "masks must be given for both sides or neither");
	if (pr->stride < dim || f->stride < dim || (pr->stride & 3) || (f->stride & 3)) return fail(MCS_ERR_INVALID, "descriptor stride must be >= dim and a multiple of 4");
	if (rule != MCS_WINDOW_INITIALIZE && bestMode != 1 && !f->assigned) return fail(MCS_ERR_INVALID, "frame->assigned is required");
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (int r = ctx_join_greedy(c, s)) return r;   // the frame's arrays may come from a search whose greedy pass runs on the side stream
	const bool havingMasks = pr->mask != nullptr;
	const size_t np = pr->n, nf = f->n;
	ProjArgs a{};
	a.rule = (int)rule; a.cap = kProjListK;
	a.nproj = pr->n; a.pstride = pr->stride; a.nfeat = f->n; a.fstride = f->stride; a.nrCams = f->nr_cams;
	a.ratio = nnratio; a.dim = dim; a.th = 1.0;
	a.thHigh = havingMasks ? (int)floor(1.5 * dim) : 3 * dim;   // TH_HIGH_ / TH_LOW_ (src/cORBmatcher.cpp:46-65)
	a.thLow = havingMasks ? (int)floor((double)dim) : 2 * dim;
	if (bestMode) a.thHigh = maxDist;
	Staging st(c, kind == MCS_MEM_HOST);
	stage_probes_frame(st, a, pr->cam, pr->desc, pr->mask, f, match, nmatches);
	st.scratch(&a.owner, nf * 4); st.scratch(&a.mdist, nf * 4);
	if (!f->assigned) st.scratch(&a.assigned, nf);   // nobody's taken yet: zeroed below
	st.in(&a.px, pr->x, np * 8); st.in(&a.py, pr->y, np * 8); st.in(&a.rad, pr->radius, np * 8); st.in(&a.minLvl, pr->min_level, np * 4); st.in(&a.maxLvl, pr->max_level, np * 4);
	int* ddist = nullptr;
	if (dist) st.out(&ddist, dist, np * 4);
	if (rule == MCS_WINDOW_INITIALIZE && pr->accepted_out != nullptr && bestMode == 0) st.out(&a.accepted, pr->accepted_out, np * 4);
	if (int r = st.commit()) return r;
	if (!f->assigned && nf) HIPCHK(hipMemsetAsync(a.assigned, 0, nf, s));
	if (pr->n > 0) {
		if (bestMode) launch_window_best(a, bestMode == 2, ddist, s);
		else { c->tic("win_candidates"); launch_proj_candidates(a, s); c->toc("win_candidates"); c->tic("win_greedy"); launch_proj_greedy(a, s); c->toc("win_greedy"); }
	}
	else HIPCHK(hipMemsetAsync(a.nmatches, 0, 4, s));
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_window_match(mcs_ctx* c, const mcs_window_probes* pr, const mcs_frame_view* f, mcs_window_rule rule, double nnratio, int dim, mcs_mem_kind kind,
                     int32_t* match, int32_t* nmatches) {
	return window_common(c, pr, f, rule, nnratio, dim, kind, match, nmatches, 0, 0, nullptr);
}

int mcs_window_best(mcs_ctx* c, const mcs_window_probes* pr, const mcs_frame_view* f, int max_dist, int skip_taken, int dim, mcs_mem_kind kind,
                    int32_t* match, int32_t* dist, int32_t* nmatches) {
	if (max_dist < 0) return fail(MCS_ERR_INVALID, "max_dist must be >= 0");
	return window_common(c, pr, f, MCS_WINDOW_BEST, 1.0, dim, kind, match, nmatches, skip_taken ? 2 : 1, max_dist, dist);
}

int mcs_world_to_cam(mcs_ctx* c, const double* MtMc_inv, const mcs_ocam* cams, int nr_cams, const uint8_t* const* mirror_masks, const double* pts3,
                     const int32_t* cam, int n, mcs_mem_kind kind, double* uv, uint8_t* flags) {
	if (!c || !MtMc_inv || !cams || !pts3 || !cam || !uv || !flags) return fail(MCS_ERR_INVALID, "null argument");
	if (nr_cams < 1 || n < 0) return fail(MCS_ERR_INVALID, "bad sizes");
	HIPCHK(hipSetDevice(c->device));
	std::vector<OcamDev> hc(nr_cams);
	std::vector<int> w(nr_cams), h(nr_cams);
	for (int i = 0; i < nr_cams; ++i) {
		if (int r = ocam_to_dev(cams[i], &hc[i])) return r;
		if (cams[i].width < 1 || cams[i].height < 1) return fail(MCS_ERR_INVALID, "bad image size");
		w[i] = cams[i].width; h[i] = cams[i].height;
	}
	WorldToCamArgs a{};
	a.n = n;
	Staging st(c, kind == MCS_MEM_HOST);
	// the matrices / calibrations are host values for either kind (they are the camera system's state, a few hundred bytes)
	st.upload(&a.M, MtMc_inv, (size_t)nr_cams * 128); st.upload(&a.cams, hc.data(), sizeof(OcamDev) * nr_cams);
	st.upload(&a.width, w.data(), 4 * (size_t)nr_cams); st.upload(&a.height, h.data(), 4 * (size_t)nr_cams);
	std::vector<const uint8_t*> mp(nr_cams, nullptr);
	if (mirror_masks) {
		for (int i = 0; i < nr_cams; ++i) st.in(&mp[i], mirror_masks[i], (size_t)w[i] * h[i]);
		st.upload(&a.masks, mp.data(), sizeof(void*) * nr_cams);   // commit() binds mp[] before it reads the sources
	}
	st.in(&a.pts, pts3, (size_t)n * 24); st.in(&a.pcam, cam, (size_t)n * 4); st.out(&a.uv, uv, (size_t)n * 16); st.out(&a.flags, flags, (size_t)n);
	if (int r = st.commit()) return r;
	launch_world_to_cam(a, c->stream);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

// ---------------------------------------------------------------------------------------------- cTracking::SearchReferencePointsInFrustum
// frame == nullptr: mcs_frustum (src/cMultiFrame.cpp:218-270 over the loop src/cTracking.cpp:981-999); else the function from :978 on.
static int local_points_common(mcs_ctx* c, const mcs_local_points* pts, const mcs_rig_view* rig, const double* scales, int nlevels, const mcs_track_state* stt,
                               const uint8_t* desc, const uint8_t* mask, int stride, const mcs_frame_view* f, double th, double nnratio, int dim, mcs_mem_kind kind,
                               int32_t* match, int32_t* nmatches, int32_t* nToMatch, int32_t* visibleInc) {
	const bool search = f != nullptr;
	if (!c || !pts || !rig || !stt || !nToMatch) return fail(MCS_ERR_INVALID, "null argument");
	if (search && (!match || !nmatches)) return fail(MCS_ERR_INVALID, "null argument");
	if (pts->n < 0 || rig->nr_cams < 1 || rig->nr_cams > 32 || (long long)pts->n * rig->nr_cams > 0x7FFFFFFFll / kProjListK) return fail(MCS_ERR_INVALID, "bad sizes");
	if (nlevels < 1 || nlevels > MCS_MAX_LEVELS) return fail(MCS_ERR_INVALID, "bad sizes");
	if (search) {
		if (dim != 16 && dim != 32 && dim != 64) return fail(MCS_ERR_INVALID, "dim must be 16, 32 or 64");
		if (f->n < 0 || f->n > 65536 || f->nr_cams != rig->nr_cams) return fail(MCS_ERR_INVALID, "bad sizes (frame features must be <= 65536)");
		if ((mask == nullptr) != (f->mask == nullptr)) return fail(MCS_ERR_INVALID, "masks must be given for both sides or neither");
		if (stride < dim || f->stride < dim || (stride & 3) || (f->stride & 3)) return fail(MCS_ERR_INVALID, "descriptor stride must be >= dim and a multiple of 4");
		if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the frustum test and the search run in order: switch deferred searches off (mcs_ctx_set_async_search)");
	}
	const int np = pts->n, nr = rig->nr_cams;
	const size_t ns = (size_t)np * nr;
	if (np > 0) {
		if (!pts->pos || !pts->normal || !pts->min_dist || !pts->max_dist || !pts->flags || !rig->MtMc_inv || !rig->MtMc || !rig->cams || !scales || !visibleInc ||
		    !stt->in_view || !stt->proj_x || !stt->proj_y || !stt->level || !stt->view_cos)
			return fail(MCS_ERR_INVALID, "null argument");
		if (search && (!desc || !f->width || !f->height || (f->n > 0 && (!f->keys || !f->desc || !f->cam || !f->assigned)))) return fail(MCS_ERR_INVALID, "null argument");
	}
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (np == 0) {   // nothing to project: nToMatch = 0, so nothing is searched either (:1001)
		if (kind == MCS_MEM_HOST) { *nToMatch = 0; if (search) *nmatches = 0; return MCS_OK; }
		HIPCHK(hipMemsetAsync(nToMatch, 0, 4, s));
		if (search) HIPCHK(hipMemsetAsync(nmatches, 0, 4, s));
		return MCS_OK;
	}
	if (kind == MCS_MEM_HOST) {   // what the kernels index with (device kind: the caller's contract)
		for (int k = 0; k < nr; ++k) {
			if (rig->cams[k].invP_deg < 1 || rig->cams[k].invP_deg > MCS_MAX_POLY) return fail(MCS_ERR_INVALID, "bad polynomial degree");
			if (rig->cams[k].width < 1 || rig->cams[k].height < 1) return fail(MCS_ERR_INVALID, "bad image size");
			if (rig->mirror_masks && !rig->mirror_masks[k]) return fail(MCS_ERR_INVALID, "null mirror mask");
		}
		if (search)
			for (int i = 0; i < np; ++i) {
				if (pts->flags[i] != MCS_LP_SEEN) continue;   // the stale slots SearchByProjection reads
				for (int k = 0; k < nr; ++k)
					if (stt->in_view[(size_t)i * nr + k] && (stt->level[(size_t)i * nr + k] < 0 || stt->level[(size_t)i * nr + k] >= nlevels))
						return fail(MCS_ERR_INVALID, "projection level outside [0, nlevels)");
			}
	}
	if (int r = ctx_join_greedy(c, s)) return r;   // the frame's arrays may come from a search whose greedy pass runs on the side stream
	// per-slot scratch, in the context's own buffer for either kind (struct mcs_ctx)
	FrustumArgs fa{};
	fa.npoints = np; fa.nrCams = nr; fa.nlevels = nlevels;
	ProjArgs a{};
	Layout lay;   // the pieces of the search keep their places without it, and bind nothing
	lay.piece(&fa.fresh, ns); lay.piece(search ? &fa.active : nullptr, search ? ns : 0); lay.piece(search ? &fa.pcam : nullptr, search ? ns * 4 : 0);
	lay.piece(search ? &a.counts : nullptr, search ? ns * 4 : 0); lay.piece(search ? &a.lists : nullptr, search ? ns * kProjListK * 8 : 0);
	HIPCHK(c->lmBuf.reserve(lay.total));
	lay.place(c->lmBuf.p);
	Staging st(c, kind == MCS_MEM_HOST);
	st.in(&fa.pos, pts->pos, (size_t)np * 24); st.in(&fa.normal, pts->normal, (size_t)np * 24); st.in(&fa.minDist, pts->min_dist, (size_t)np * 8);
	st.in(&fa.maxDist, pts->max_dist, (size_t)np * 8); st.in(&fa.flags, pts->flags, (size_t)np);
	st.in(&fa.MtMcInv, rig->MtMc_inv, (size_t)nr * 128); st.in(&fa.MtMc, rig->MtMc, (size_t)nr * 128); st.in(&fa.cams, rig->cams, (size_t)nr * sizeof(mcs_ocam));
	std::vector<const uint8_t*> mp(nr, nullptr);
	if (kind == MCS_MEM_HOST && rig->mirror_masks) {
		for (int k = 0; k < nr; ++k) st.in(&mp[k], rig->mirror_masks[k], (size_t)rig->cams[k].width * rig->cams[k].height);
		st.upload(&fa.masks, mp.data(), sizeof(void*) * nr);   // commit() binds mp[] before it reads the sources
	} else fa.masks = rig->mirror_masks;
	st.inout(&fa.inView, stt->in_view, ns); st.inout(&fa.projX, stt->proj_x, ns * 8); st.inout(&fa.projY, stt->proj_y, ns * 8);
	st.inout(&fa.level, stt->level, ns * 4); st.inout(&fa.viewCos, stt->view_cos, ns * 8);
	st.out(&fa.visibleInc, visibleInc, (size_t)np * 4); st.out(&fa.nToMatch, nToMatch, 4);
	if (search) {
		const size_t nf = f->n, nc = f->nr_cams;
		a.nproj = (int)ns; a.pstride = stride; a.nfeat = f->n; a.fstride = f->stride; a.nrCams = f->nr_cams;
		a.th = th; a.ratio = nnratio; a.dim = dim; a.rule = 0; a.cap = kProjListK;
		a.thHigh = mask ? (int)floor(1.5 * dim) : 3 * dim;   // TH_HIGH_ (src/cORBmatcher.cpp:46-65)
		a.pcam = fa.pcam; a.active = fa.active; a.rowDiv = nr;
		st.in(&a.pdesc, desc, (size_t)np * stride); st.in(&a.pmask, mask, (size_t)np * stride);
		st.in(&a.keys, f->keys, nf * sizeof(mcs_keypoint)); st.in(&a.fdesc, f->desc, nf * f->stride); st.in(&a.fmask, f->mask, nf * f->stride); st.in(&a.fcam, f->cam, nf * 4);
		st.in(&a.width, f->width, nc * 4); st.in(&a.height, f->height, nc * 4);
		st.inout(&a.assigned, f->assigned, nf);
		st.out(&a.match, match, ns * 4); st.out(&a.nmatches, nmatches, 4);
	}
	st.in(&fa.scales, scales, (size_t)nlevels * 8);
	if (int r = st.commit()) return r;
	c->tic("frustum"); launch_frustum(fa, s); c->toc("frustum");
	if (search) {
		a.px = fa.projX; a.py = fa.projY; a.vcos = fa.viewCos; a.level = fa.level; a.scales = fa.scales;
		// grids sized by the host-known slot count; an idle slot leaves at once (k_proj_candidates) and the greedy pass resolves it to -1
		c->tic("lm_candidates"); launch_proj_candidates(a, s); c->toc("lm_candidates");
		c->tic("lm_greedy"); launch_proj_greedy(a, s); c->toc("lm_greedy");
		c->lastResultStream = s;   // every output is complete on the context's stream
	}
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_frustum(mcs_ctx* c, const mcs_local_points* pts, const mcs_rig_view* rig, const double* scale_factors, int nlevels, const mcs_track_state* state,
                mcs_mem_kind kind, int32_t* visible_inc, int32_t* n_to_match) {
	return local_points_common(c, pts, rig, scale_factors, nlevels, state, nullptr, nullptr, 0, nullptr, 0.0, 0.0, 0, kind, nullptr, nullptr, n_to_match, visible_inc);
}

int mcs_search_local_points(mcs_ctx* c, const mcs_local_points* pts, const mcs_rig_view* rig, const mcs_track_state* state, const uint8_t* desc, const uint8_t* mask,
                            int stride, const mcs_frame_view* frame, double th, double nnratio, int dim, mcs_mem_kind kind, int32_t* match, int32_t* nmatches,
                            int32_t* n_to_match, int32_t* visible_inc) {
	if (!frame) return fail(MCS_ERR_INVALID, "null argument");
	return local_points_common(c, pts, rig, frame->scale_factors, frame->nlevels, state, desc, mask, stride, frame, th, nnratio, dim, kind, match, nmatches,
	                           n_to_match, visible_inc);
}

// ---------------------------------------------------------------------------------------------- cTracking::TrackWithMotionModel / TrackPreviousFrame
// rig != nullptr: SearchByProjection(CurrentFrame, LastFrame, th) (src/cORBmatcher.cpp:1990-2118), tf = LastFrame, f = CurrentFrame;
// else WindowSearch(F1, F2, ...) (:326-473), tf = F1, f = F2.  matchFeat[f->n] = tracked feature per frame feature, featPoints[f->n] = its point id.
static int tracked_common(mcs_ctx* c, const mcs_tracked_frame* tf, const mcs_point_table* pts, const mcs_rig_view* rig, const mcs_frame_view* f, double th,
                          int windowSize, int minLevel, int maxLevel, double nnratio, int dim, int checkOrientation, mcs_mem_kind kind, int32_t* matchFeat,
                          int32_t* featPoints, int32_t* nmatches) {
	const bool project = rig != nullptr;
	if (!c || !tf || !pts || !f || !matchFeat || !nmatches) return fail(MCS_ERR_INVALID, "null argument");
	if (dim != 16 && dim != 32 && dim != 64) return fail(MCS_ERR_INVALID, "dim must be 16, 32 or 64");
	if (tf->n < 0 || tf->n > 65536 || f->n < 0 || f->n > 65536 || pts->n < 0 || f->nr_cams < 1 || f->nr_cams > 32)
		return fail(MCS_ERR_INVALID, "bad sizes (frame features must be <= 65536)");
	if (project && (rig->nr_cams != f->nr_cams || f->nlevels < 1 || f->nlevels > MCS_MAX_LEVELS)) return fail(MCS_ERR_INVALID, "bad sizes (rig and frame must agree on the cameras)");
	if ((tf->mask == nullptr) != (f->mask == nullptr)) return fail(MCS_ERR_INVALID, "masks must be given for both sides or neither");
	if (tf->stride < dim || f->stride < dim || (tf->stride & 3) || (f->stride & 3)) return fail(MCS_ERR_INVALID, "descriptor stride must be >= dim and a multiple of 4");
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the probes and the search run in order: switch deferred searches off (mcs_ctx_set_async_search)");
	const int np = tf->n, nf = f->n, nr = f->nr_cams;
	if (np > 0 && nf > 0) {
		if (!tf->keys || !tf->desc || !tf->cam || !tf->points || !f->keys || !f->desc || !f->cam || !f->width || !f->height || (pts->n > 0 && (!pts->pos || !pts->flags)))
			return fail(MCS_ERR_INVALID, "null argument");
		if (project && (!rig->MtMc_inv || !rig->cams || !f->scale_factors || !f->assigned)) return fail(MCS_ERR_INVALID, "null argument");
	}
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (np == 0 || nf == 0) {   // nobody to track or nothing to find: every entry -1 (WindowSearch starts vpMapPointMatches2 from NULLs), no match
		if (kind == MCS_MEM_HOST) {
			for (int j = 0; j < nf; ++j) { matchFeat[j] = -1; if (!project && featPoints) featPoints[j] = -1; }
			*nmatches = 0;
			return MCS_OK;
		}
		if (nf > 0) HIPCHK(hipMemsetAsync(matchFeat, 0xFF, (size_t)nf * 4, s));
		if (nf > 0 && !project && featPoints) HIPCHK(hipMemsetAsync(featPoints, 0xFF, (size_t)nf * 4, s));
		HIPCHK(hipMemsetAsync(nmatches, 0, 4, s));
		c->lastResultStream = s;   // the memsets are this call's outputs
		return MCS_OK;
	}
	if (kind == MCS_MEM_HOST) {   // what the kernels index with (device kind: such a slot is idle, k_track_probes)
		if (project)
			for (int k = 0; k < nr; ++k) {
				if (rig->cams[k].invP_deg < 1 || rig->cams[k].invP_deg > MCS_MAX_POLY) return fail(MCS_ERR_INVALID, "bad polynomial degree");
				if (rig->cams[k].width < 1 || rig->cams[k].height < 1) return fail(MCS_ERR_INVALID, "bad image size");
				if (rig->mirror_masks && !rig->mirror_masks[k]) return fail(MCS_ERR_INVALID, "null mirror mask");
			}
		for (int i = 0; i < np; ++i) {
			if (tf->points[i] < 0) continue;   // NULL: nothing of this feature is read
			if (tf->points[i] >= pts->n) return fail(MCS_ERR_INVALID, "map point id outside [0, points->n)");
			if (tf->cam[i] < 0 || tf->cam[i] >= nr) return fail(MCS_ERR_INVALID, "camera index outside [0, nr_cams)");
			if (project && (tf->keys[i].octave < 0 || tf->keys[i].octave >= f->nlevels)) return fail(MCS_ERR_INVALID, "key octave outside [0, nlevels)");
		}
	}
	if (int r = ctx_join_greedy(c, s)) return r;   // the frame's arrays may come from a search whose greedy pass runs on the side stream
	// per-slot scratch, in the context's own buffer for either kind (struct mcs_ctx): a device-kind call returns while its kernels still use it
	TrackArgs t{};
	ProjArgs a{};
	TrackTailArgs tail{};
	int *matchSlot = nullptr, *removed = nullptr;
	uint8_t* taken = nullptr;
	Layout lay;
	lay.piece(&t.px, (size_t)np * 8); lay.piece(&t.py, (size_t)np * 8); lay.piece(&t.rad, (size_t)np * 8); lay.piece(&t.minLvl, (size_t)np * 4);
	lay.piece(&t.maxLvl, (size_t)np * 4); lay.piece(&t.pcam, (size_t)np * 4); lay.piece(&t.active, (size_t)np);
	lay.piece(&a.counts, (size_t)np * 4); lay.piece(&a.lists, (size_t)np * kProjListK * 8);
	lay.piece(&matchSlot, (size_t)np * 4); lay.piece(&removed, 4); lay.piece(&taken, (size_t)nf);
	HIPCHK(c->lmBuf.reserve(lay.total));
	lay.place(c->lmBuf.p);
	// the window form reads neither the rig (MtMcInv, cams, masks stay null) nor outlier, scales, nlevels and th; the projection form none of the last three
	t.n = np; t.npoints = pts->n; t.project = project ? 1 : 0; t.nrCams = nr; t.nlevels = f->nlevels; t.th = th;
	t.windowSize = (double)windowSize; t.minLevel = minLevel; t.maxLevel = maxLevel;
	Staging st(c, kind == MCS_MEM_HOST);
	st.in(&t.keys, tf->keys, (size_t)np * sizeof(mcs_keypoint)); st.in(&t.cam, tf->cam, (size_t)np * 4); st.in(&t.points, tf->points, (size_t)np * 4);
	st.in(&t.outlier, project ? tf->outlier : nullptr, (size_t)np);
	st.in(&t.pos, pts->pos, (size_t)pts->n * 24); st.in(&t.flags, pts->flags, (size_t)pts->n);
	st.in(&a.pdesc, tf->desc, (size_t)np * tf->stride); st.in(&a.pmask, tf->mask, (size_t)np * tf->stride);
	std::vector<const uint8_t*> mp(nr, nullptr);
	if (project) {
		st.in(&t.MtMcInv, rig->MtMc_inv, (size_t)nr * 128); st.in(&t.cams, rig->cams, (size_t)nr * sizeof(mcs_ocam));
		if (kind == MCS_MEM_HOST && rig->mirror_masks) {
			for (int k = 0; k < nr; ++k) st.in(&mp[k], rig->mirror_masks[k], (size_t)rig->cams[k].width * rig->cams[k].height);
			st.upload(&t.masks, mp.data(), sizeof(void*) * nr);   // commit() binds mp[] before it reads the sources
		} else t.masks = rig->mirror_masks;
		st.in(&t.scales, f->scale_factors, (size_t)f->nlevels * 8);
	}
	const bool havingMasks = tf->mask != nullptr;
	a.nproj = np; a.pstride = tf->stride; a.nfeat = nf; a.fstride = f->stride; a.nrCams = nr;
	a.th = 1.0; a.ratio = nnratio; a.dim = dim; a.rule = project ? (int)MCS_WINDOW_BEST : (int)MCS_WINDOW_RATIO; a.cap = kProjListK;
	a.thHigh = havingMasks ? (int)floor(1.5 * dim) : 3 * dim;   // TH_HIGH_ / TH_LOW_ (src/cORBmatcher.cpp:46-65)
	a.thLow = havingMasks ? (int)floor((double)dim) : 2 * dim;
	a.px = t.px; a.py = t.py; a.rad = t.rad; a.minLvl = t.minLvl; a.maxLvl = t.maxLvl; a.pcam = t.pcam; a.active = t.active; a.rowDiv = 0;
	st.in(&a.keys, f->keys, (size_t)nf * sizeof(mcs_keypoint)); st.in(&a.fdesc, f->desc, (size_t)nf * f->stride); st.in(&a.fmask, f->mask, (size_t)nf * f->stride);
	st.in(&a.fcam, f->cam, (size_t)nf * 4); st.in(&a.width, f->width, (size_t)nr * 4); st.in(&a.height, f->height, (size_t)nr * 4);
	if (project) st.inout(&a.assigned, f->assigned, (size_t)nf);
	else a.assigned = taken;   // vpMapPointMatches2 starts from NULLs (:333): F2's own matches are neither read nor written
	a.match = matchSlot;
	st.out(&a.nmatches, nmatches, 4);
	tail.matchSlot = matchSlot; tail.n = np; tail.nfeat = nf; tail.clearDropped = project ? 1 : 0;
	st.out(&tail.matchFeat, matchFeat, (size_t)nf * 4);
	if (featPoints) { if (project) st.inout(&tail.featPoints, featPoints, (size_t)nf * 4); else st.out(&tail.featPoints, featPoints, (size_t)nf * 4); }
	if (int r = st.commit()) return r;
	tail.points = t.points; tail.assigned = project ? a.assigned : nullptr; tail.removed = checkOrientation ? removed : nullptr; tail.nmatches = a.nmatches;
	if (!project) HIPCHK(hipMemsetAsync(taken, 0, (size_t)nf, s));
	c->tic("track_probes"); launch_track_probes(t, s); c->toc("track_probes");
	// grids sized by the host-known slot count; an idle slot leaves at once (k_proj_candidates) and the greedy pass resolves it to -1
	c->tic("track_candidates"); launch_proj_candidates(a, s); c->toc("track_candidates");
	c->tic("track_greedy"); launch_proj_greedy(a, s); c->toc("track_greedy");
	c->tic("track_tail");
	HIPCHK(hipMemsetAsync(tail.matchFeat, 0xFF, (size_t)nf * 4, s));
	if (!project && tail.featPoints) HIPCHK(hipMemsetAsync(tail.featPoints, 0xFF, (size_t)nf * 4, s));
	launch_track_invert(tail, s);
	if (checkOrientation) {   // :2096-2115 variant 0, :442-462 variant 1; rot = tracked angle - frame angle: the slot is the frame's feature, so swapped
		const float* angF = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.keys) + offsetof(mcs_keypoint, angle));
		const float* angT = reinterpret_cast<const float*>(reinterpret_cast<const char*>(t.keys) + offsetof(mcs_keypoint, angle));
		launch_rotation_consistency(project ? 0 : 1, angF, (int)sizeof(mcs_keypoint), angT, (int)sizeof(mcs_keypoint), nullptr, tail.matchFeat, nf, 1, removed, s);
	}
	launch_track_finish(tail, s);
	c->toc("track_tail");
	c->lastResultStream = s;   // every output is complete on the context's stream
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_search_last_frame(mcs_ctx* c, const mcs_tracked_frame* last, const mcs_point_table* pts, const mcs_rig_view* rig, const mcs_frame_view* cur, double th,
                          int dim, int check_orientation, mcs_mem_kind kind, int32_t* match_cur, int32_t* cur_points, int32_t* nmatches) {
	if (!rig) return fail(MCS_ERR_INVALID, "null argument");
	return tracked_common(c, last, pts, rig, cur, th, 0, 0, 0x7FFFFFFF, 1.0, dim, check_orientation, kind, match_cur, cur_points, nmatches);
}

int mcs_window_search_frames(mcs_ctx* c, const mcs_tracked_frame* f1, const mcs_point_table* pts, const mcs_frame_view* f2, int window_size, int min_level,
                             int max_level, double nnratio, int dim, int check_orientation, mcs_mem_kind kind, int32_t* match21, int32_t* points2,
                             int32_t* nmatches) {
	return tracked_common(c, f1, pts, nullptr, f2, 0.0, window_size, min_level, max_level, nnratio, dim, check_orientation, kind, match21, points2, nmatches);
}

int mcs_distinctive_descriptors(mcs_ctx* c, const uint8_t* desc, const uint8_t* mask, int stride, int dim, const int32_t* offsets, int npoints,
                                mcs_mem_kind kind, int32_t* best_idx) {
	if (!c || !desc || !offsets || !best_idx) return fail(MCS_ERR_INVALID, "null argument");
	if (dim != 16 && dim != 32 && dim != 64) return fail(MCS_ERR_INVALID, "dim must be 16, 32 or 64");
	if (stride < dim || (stride & 3) || npoints < 0) return fail(MCS_ERR_INVALID, "bad stride / count");
	if (npoints == 0) return MCS_OK;
	size_t rows = 0;
	if (kind == MCS_MEM_HOST) {   // (device kind: offsets are validated by the caller, and nothing is staged)
		if (offsets[0] != 0) return fail(MCS_ERR_INVALID, "offsets[0] must be 0");
		for (int k = 0; k < npoints; ++k)
			if (offsets[k + 1] < offsets[k] || offsets[k + 1] - offsets[k] > 65535) return fail(MCS_ERR_INVALID, "offsets must be non-decreasing, <= 65535 rows per map point");
		rows = (size_t)offsets[npoints];
	}
	HIPCHK(hipSetDevice(c->device));
	DistinctArgs a{};
	a.stride = stride; a.dim = dim; a.npoints = npoints;
	Staging st(c, kind == MCS_MEM_HOST);
	st.in(&a.desc, desc, rows * stride); st.in(&a.mask, mask, rows * stride); st.in(&a.offsets, offsets, ((size_t)npoints + 1) * 4);
	st.out(&a.bestIdx, best_idx, (size_t)npoints * 4);
	if (int r = st.commit()) return r;
	launch_distinct(a, c->stream);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

namespace mcs { void launch_selftest_recip(unsigned long long seed, int n, int* mismatches, hipStream_t s); }

int mcs_selftest_shared_reciprocal(mcs_ctx* c, uint64_t seed, int n, int32_t* mismatches) {
	if (!c || !mismatches || n < 1) return fail(MCS_ERR_INVALID, "bad argument");
	HIPCHK(hipSetDevice(c->device));
	int* d = nullptr;
	HIPCHK(hipMalloc((void**)&d, 4));
	(void)hipMemsetAsync(d, 0, 4, c->stream);
	launch_selftest_recip(seed, n, d, c->stream);
	const hipError_t e1 = hipGetLastError();
	const hipError_t e2 = hipMemcpyAsync(mismatches, d, 4, hipMemcpyDeviceToHost, c->stream);
	const hipError_t e3 = hipStreamSynchronize(c->stream);
	(void)hipFree(d);
	if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return fail(MCS_ERR_HIP, "selftest kernel failed");
	return MCS_OK;
}

int mcs_rotation_consistency(mcs_ctx* c, int variant, const float* angle_slot, int stride_slot, const float* angle_partner, int stride_partner,
                             const int32_t* accepted, int32_t* match, int n, int n_partner, int swapped, mcs_mem_kind kind, int32_t* removed) {
	if (!c || !angle_slot || !angle_partner || !match || !removed) return fail(MCS_ERR_INVALID, "null argument");
	if (variant < 0 || variant > 3 || n < 0 || n_partner < 0 || stride_slot < 4 || stride_partner < 4 || (stride_slot & 3) || (stride_partner & 3))
		return fail(MCS_ERR_INVALID, "bad variant / sizes / strides");
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (int r = ctx_join_greedy(c, s)) return r;   // `match` may come from a search whose greedy pass runs on the side stream
	const size_t bs = (size_t)n * stride_slot, bp = (size_t)n_partner * stride_partner;
	const float *dSlot = nullptr, *dPartner = nullptr; const int* dAcc = nullptr; int *dMatch = nullptr, *dRemoved = nullptr;
	Staging st(c, kind == MCS_MEM_HOST);
	st.in(&dSlot, angle_slot, bs > 0 ? bs - (stride_slot - 4) : 0); st.in(&dPartner, angle_partner, bp > 0 ? bp - (stride_partner - 4) : 0);   // the last keypoint's tail may not be readable
	st.in(&dAcc, accepted, (size_t)n * 4); st.inout(&dMatch, match, (size_t)n * 4); st.out(&dRemoved, removed, 4);
	if (int r = st.commit()) return r;
	launch_rotation_consistency(variant, dSlot, stride_slot, dPartner, stride_partner, dAcc, dMatch, n, swapped, dRemoved, s);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}
