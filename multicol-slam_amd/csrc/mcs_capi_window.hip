// mcs_capi_window.hip — C ABI of the grid-window matchers over probes the caller lists (SearchByProjection(F, mapPoints), the explicit-window rules, the
// closest feature per window) and of the two helpers composed around them: the projection that makes the probes and the rotation filter that follows them
// (include/mcs_c.h: mcs_search_by_projection, mcs_window_match, mcs_window_best, mcs_world_to_cam, mcs_rotation_consistency).  The searches that make their own
// probes on the device are in mcs_capi_track.hip; the argument checks of both files in mcs_window_guard.hip.  Kernels: mcs_project.hip.
#include "mcs_window.h"

using namespace mcs;

namespace mcs {
void launch_window_best(const ProjArgs& a, bool skipTaken, int* outDist, hipStream_t s);
void launch_rotation_consistency(int variant, const float* angleSlot, int strideSlot, const float* anglePartner, int stridePartner, const int* accepted, int* match,
                                 int n, int swapped, int* removedOut, hipStream_t s);
}

// What the projection search and the window matchers share: the candidate lists, the probes' camera / descriptor / mask, the frame's arrays and the outputs.
// The scratch makes every call claim the context's block, so a device-kind call ends with a stream synchronisation too (these rows are not bench paths).
static void stage_probes_frame(Staging& st, ProjArgs& a, const int32_t* pcam, const uint8_t* pdesc, const uint8_t* pmask, const mcs_frame_view* f, Assigned how,
                               int32_t* match, int32_t* nmatches) {
	const size_t np = a.nproj;
	st.scratch(&a.lists, np * kProjListK * 8); st.scratch(&a.counts, np * 4);
	st.in(&a.pcam, pcam, np * 4); st.in(&a.pdesc, pdesc, np * a.pstride); st.in(&a.pmask, pmask, np * a.pstride);
	stage_frame(st, a, f, how);
	st.out(&a.match, match, np * 4); st.out(&a.nmatches, nmatches, 4);
}

int mcs_search_by_projection(mcs_ctx* c, const mcs_projection_set* mp, const mcs_frame_view* f, double th, double nnratio, int dim, mcs_mem_kind kind,
                             int32_t* match, int32_t* nmatches) {
	if (int r = guard_search_by_projection(c, mp, f, dim, kind == MCS_MEM_HOST, match, nmatches)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (int r = ctx_join_greedy(c, s)) return r;   // the frame's arrays may come from a search whose greedy pass runs on the side stream
	ProjArgs a{};
	a.nproj = mp->n; a.pstride = mp->stride;
	a.th = th; a.ratio = nnratio; a.dim = dim; a.rule = 0; a.cap = kProjListK;
	a.thHigh = window_thresholds(dim, mp->mask != nullptr).high;
	const size_t np = mp->n;
	Staging st(c, kind == MCS_MEM_HOST);
	stage_probes_frame(st, a, mp->cam, mp->desc, mp->mask, f, Assigned::Callers, match, nmatches);
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
	if (int r = guard_window(c, pr, f, rule, dim, bestMode, maxDist, match, nmatches)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (int r = ctx_join_greedy(c, s)) return r;   // the frame's arrays may come from a search whose greedy pass runs on the side stream
	const size_t np = pr->n, nf = f->n;
	ProjArgs a{};
	a.rule = (int)rule; a.cap = kProjListK;
	a.nproj = pr->n; a.pstride = pr->stride;
	a.ratio = nnratio; a.dim = dim; a.th = 1.0;
	const Thresholds th = window_thresholds(dim, pr->mask != nullptr);
	a.thHigh = bestMode ? maxDist : th.high; a.thLow = th.low;
	Staging st(c, kind == MCS_MEM_HOST);
	stage_probes_frame(st, a, pr->cam, pr->desc, pr->mask, f, f->assigned ? Assigned::Callers : Assigned::Scratch, match, nmatches);   // scratch: nobody's taken yet
	st.scratch(&a.owner, nf * 4); st.scratch(&a.mdist, nf * 4);
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
	return window_common(c, pr, f, MCS_WINDOW_BEST, 1.0, dim, kind, match, nmatches, skip_taken ? 2 : 1, max_dist, dist);
}

int mcs_world_to_cam(mcs_ctx* c, const double* MtMc_inv, const mcs_ocam* cams, int nr_cams, const uint8_t* const* mirror_masks, const double* pts3,
                     const int32_t* cam, int n, mcs_mem_kind kind, double* uv, uint8_t* flags) {
	if (int r = guard_world_to_cam(c, MtMc_inv, cams, nr_cams, pts3, cam, n, uv, flags)) return r;
	HIPCHK(hipSetDevice(c->device));
	std::vector<OcamDev> hc(nr_cams);
	std::vector<int> w(nr_cams), h(nr_cams);
	for (int i = 0; i < nr_cams; ++i) {
		if (int r = ocam_to_dev(cams[i], &hc[i])) return r;
		if (int r = guard_image_size(cams[i])) return r;
		w[i] = cams[i].width; h[i] = cams[i].height;
	}
	WorldToCamArgs a{};
	a.n = n;
	Staging st(c, kind == MCS_MEM_HOST);
	// the matrices / calibrations / the table of mask pointers are host values for either kind (they are the camera system's state, a few hundred bytes)
	st.upload(&a.M, MtMc_inv, (size_t)nr_cams * 128); st.upload(&a.cams, hc.data(), sizeof(OcamDev) * nr_cams);
	st.upload(&a.width, w.data(), 4 * (size_t)nr_cams); st.upload(&a.height, h.data(), 4 * (size_t)nr_cams);
	std::vector<const uint8_t*> mp(nr_cams, nullptr);
	stage_mirror_masks(st, &a.masks, mirror_masks, true, cams, nr_cams, mp);
	st.in(&a.pts, pts3, (size_t)n * 24); st.in(&a.pcam, cam, (size_t)n * 4); st.out(&a.uv, uv, (size_t)n * 16); st.out(&a.flags, flags, (size_t)n);
	if (int r = st.commit()) return r;
	launch_world_to_cam(a, c->stream);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_rotation_consistency(mcs_ctx* c, int variant, const float* angle_slot, int stride_slot, const float* angle_partner, int stride_partner,
                             const int32_t* accepted, int32_t* match, int n, int n_partner, int swapped, mcs_mem_kind kind, int32_t* removed) {
	if (int r = guard_rotation_consistency(c, variant, angle_slot, stride_slot, angle_partner, stride_partner, match, n, n_partner, removed)) return r;
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
