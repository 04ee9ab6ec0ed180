// mcs_capi_track.hip — C ABI of the tracker's searches that make their own probes on the device and hand them to the window matcher in the same call: the search
// step of TrackLocalMap (include/mcs_c.h: mcs_frustum, mcs_search_local_points) and the frame-to-frame searches of TrackWithMotionModel / TrackPreviousFrame
// (mcs_search_last_frame, mcs_window_search_frames).  Every device-kind call only enqueues: its per-slot scratch is the context's lmBuf, not the staging block.
// Argument checks: mcs_window_guard.hip.  Kernels: mcs_frustum.hip, mcs_lastframe.hip, mcs_project.hip.
#include "mcs_window.h"

using namespace mcs;

namespace mcs {
void launch_rotation_consistency(int variant, const float* angleSlot, int strideSlot, const float* anglePartner, int stridePartner, const int* accepted, int* match,
                                 int n, int swapped, int* removedOut, hipStream_t s);
}

// ---------------------------------------------------------------------------------------------- cTracking::SearchReferencePointsInFrustum
// LocalCall (mcs_window.h), f == nullptr: mcs_frustum (src/cMultiFrame.cpp:218-270 over the loop src/cTracking.cpp:981-999); else the function from :978 on.

// nothing to project: nToMatch = 0, so nothing is searched either (:1001)
static int local_empty(const LocalCall& q, hipStream_t s) {
	if (q.kind == MCS_MEM_HOST) { *q.nToMatch = 0; if (q.search()) *q.nmatches = 0; return MCS_OK; }
	HIPCHK(hipMemsetAsync(q.nToMatch, 0, 4, s));
	if (q.search()) HIPCHK(hipMemsetAsync(q.nmatches, 0, 4, s));
	return MCS_OK;
}

// per-slot scratch, in the context's own buffer for either kind (struct mcs_ctx)
static int local_layout(mcs_ctx* c, const LocalCall& q, FrustumArgs& fa, ProjArgs& a) {
	const bool search = q.search();
	const size_t ns = q.slots();
	Layout lay;   // the pieces of the search keep their places without it, and bind nothing
	lay.piece(&fa.fresh, ns); lay.piece(search ? &fa.active : nullptr, search ? ns : 0); lay.piece(search ? &fa.pcam : nullptr, search ? ns * 4 : 0);
	lay.piece(search ? &a.counts : nullptr, search ? ns * 4 : 0); lay.piece(search ? &a.lists : nullptr, search ? ns * kProjListK * 8 : 0);
	HIPCHK(c->lmBuf.reserve(lay.total));
	lay.place(c->lmBuf.p);
	return MCS_OK;
}

static void local_stage(Staging& st, const LocalCall& q, FrustumArgs& fa, ProjArgs& a, std::vector<const uint8_t*>& maskSlots) {
	const mcs_local_points* pts = q.pts; const mcs_rig_view* rig = q.rig; const mcs_track_state* stt = q.stt;
	const size_t np = pts->n, nr = rig->nr_cams, ns = q.slots();
	fa.npoints = pts->n; fa.nrCams = rig->nr_cams; fa.nlevels = q.nlevels;
	st.in(&fa.pos, pts->pos, np * 24); st.in(&fa.normal, pts->normal, np * 24); st.in(&fa.minDist, pts->min_dist, np * 8);
	st.in(&fa.maxDist, pts->max_dist, np * 8); st.in(&fa.flags, pts->flags, np);
	st.in(&fa.MtMcInv, rig->MtMc_inv, nr * 128); st.in(&fa.MtMc, rig->MtMc, nr * 128); st.in(&fa.cams, rig->cams, nr * sizeof(mcs_ocam));
	stage_mirror_masks(st, &fa.masks, rig->mirror_masks, q.kind == MCS_MEM_HOST, rig->cams, rig->nr_cams, maskSlots);
	st.inout(&fa.inView, stt->in_view, ns); st.inout(&fa.projX, stt->proj_x, ns * 8); st.inout(&fa.projY, stt->proj_y, ns * 8);
	st.inout(&fa.level, stt->level, ns * 4); st.inout(&fa.viewCos, stt->view_cos, ns * 8);
	st.out(&fa.visibleInc, q.visibleInc, np * 4); st.out(&fa.nToMatch, q.nToMatch, 4);
	if (q.search()) {
		a.nproj = (int)ns; a.pstride = q.stride;
		a.th = q.th; a.ratio = q.nnratio; a.dim = q.dim; a.rule = 0; a.cap = kProjListK;
		a.thHigh = window_thresholds(q.dim, q.mask != nullptr).high;
		a.pcam = fa.pcam; a.active = fa.active; a.rowDiv = rig->nr_cams;
		st.in(&a.pdesc, q.desc, np * q.stride); st.in(&a.pmask, q.mask, np * q.stride);
		stage_frame(st, a, q.f, Assigned::Callers);
		st.out(&a.match, q.match, ns * 4); st.out(&a.nmatches, q.nmatches, 4);
	}
	st.in(&fa.scales, q.scales, (size_t)q.nlevels * 8);
}

static void local_launch(mcs_ctx* c, bool search, const FrustumArgs& fa, ProjArgs& a, hipStream_t s) {
	c->tic("frustum"); launch_frustum(fa, s); c->toc("frustum");
	if (!search) return;
	a.px = fa.projX; a.py = fa.projY; a.vcos = fa.viewCos; a.level = fa.level; a.scales = fa.scales;
	// grids sized by the host-known slot count; an idle slot leaves at once (k_proj_candidates) and the greedy pass resolves it to -1
	c->tic("lm_candidates"); launch_proj_candidates(a, s); c->toc("lm_candidates");
	c->tic("lm_greedy"); launch_proj_greedy(a, s); c->toc("lm_greedy");
	c->lastResultStream = s;   // every output is complete on the context's stream
}

static int local_points_common(mcs_ctx* c, const LocalCall& q) {
	if (int r = guard_local_points(c, q, c && c->asyncSearch)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (q.pts->n == 0) return local_empty(q, s);
	if (q.kind == MCS_MEM_HOST)
		if (int r = guard_local_points_content(q)) return r;
	if (int r = ctx_join_greedy(c, s)) return r;   // the frame's arrays may come from a search whose greedy pass runs on the side stream
	FrustumArgs fa{};
	ProjArgs a{};
	if (int r = local_layout(c, q, fa, a)) return r;
	Staging st(c, q.kind == MCS_MEM_HOST);
	std::vector<const uint8_t*> maskSlots(q.rig->nr_cams, nullptr);
	local_stage(st, q, fa, a, maskSlots);
	if (int r = st.commit()) return r;
	local_launch(c, q.search(), fa, a, s);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_frustum(mcs_ctx* c, const mcs_local_points* pts, const mcs_rig_view* rig, const double* scale_factors, int nlevels, const mcs_track_state* state,
                mcs_mem_kind kind, int32_t* visible_inc, int32_t* n_to_match) {
	return local_points_common(c, LocalCall{pts, rig, scale_factors, nlevels, state, nullptr, nullptr, 0, nullptr, 0.0, 0.0, 0, kind, nullptr, nullptr, n_to_match, visible_inc});
}

int mcs_search_local_points(mcs_ctx* c, const mcs_local_points* pts, const mcs_rig_view* rig, const mcs_track_state* state, const uint8_t* desc, const uint8_t* mask,
                            int stride, const mcs_frame_view* frame, double th, double nnratio, int dim, mcs_mem_kind kind, int32_t* match, int32_t* nmatches,
                            int32_t* n_to_match, int32_t* visible_inc) {
	if (!frame) return null_argument();
	return local_points_common(c, LocalCall{pts, rig, frame->scale_factors, frame->nlevels, state, desc, mask, stride, frame, th, nnratio, dim, kind, match, nmatches,
	                                        n_to_match, visible_inc});
}

// ---------------------------------------------------------------------------------------------- cTracking::TrackWithMotionModel / TrackPreviousFrame
// rig != nullptr: SearchByProjection(CurrentFrame, LastFrame, th) (src/cORBmatcher.cpp:1990-2118), tf = LastFrame, f = CurrentFrame;
// else WindowSearch(F1, F2, ...) (:326-473), tf = F1, f = F2.  matchFeat[f->n] = tracked feature per frame feature, featPoints[f->n] = its point id (TrackedCall).
struct TrackedPieces { int* matchSlot = nullptr; int* removed = nullptr; uint8_t* taken = nullptr; };   // of lmBuf, beside those bound into the kernels' arguments

// nobody to track or nothing to find: every entry -1 (WindowSearch starts vpMapPointMatches2 from NULLs), no match
static int tracked_empty(mcs_ctx* c, const TrackedCall& q, hipStream_t s) {
	const int nf = q.f->n;
	const bool points = !q.project() && q.featPoints;
	if (q.kind == MCS_MEM_HOST) {
		for (int j = 0; j < nf; ++j) { q.matchFeat[j] = -1; if (points) q.featPoints[j] = -1; }
		*q.nmatches = 0;
		return MCS_OK;
	}
	if (nf > 0) HIPCHK(hipMemsetAsync(q.matchFeat, 0xFF, (size_t)nf * 4, s));
	if (nf > 0 && points) HIPCHK(hipMemsetAsync(q.featPoints, 0xFF, (size_t)nf * 4, s));
	HIPCHK(hipMemsetAsync(q.nmatches, 0, 4, s));
	c->lastResultStream = s;   // the memsets are this call's outputs
	return MCS_OK;
}

// per-slot scratch, in the context's own buffer for either kind (struct mcs_ctx): a device-kind call returns while its kernels still use it
static int tracked_layout(mcs_ctx* c, const TrackedCall& q, TrackArgs& t, ProjArgs& a, TrackedPieces& p) {
	const size_t np = q.tf->n, nf = q.f->n;
	Layout lay;
	lay.piece(&t.px, np * 8); lay.piece(&t.py, np * 8); lay.piece(&t.rad, np * 8); lay.piece(&t.minLvl, np * 4);
	lay.piece(&t.maxLvl, np * 4); lay.piece(&t.pcam, np * 4); lay.piece(&t.active, np);
	lay.piece(&a.counts, np * 4); lay.piece(&a.lists, np * kProjListK * 8);
	lay.piece(&p.matchSlot, np * 4); lay.piece(&p.removed, 4); lay.piece(&p.taken, nf);
	HIPCHK(c->lmBuf.reserve(lay.total));
	lay.place(c->lmBuf.p);
	return MCS_OK;
}

static void tracked_stage(Staging& st, const TrackedCall& q, const TrackedPieces& p, TrackArgs& t, ProjArgs& a, TrackTailArgs& tail,
                          std::vector<const uint8_t*>& maskSlots) {
	const mcs_tracked_frame* tf = q.tf; const mcs_point_table* pts = q.pts; const mcs_rig_view* rig = q.rig; const mcs_frame_view* f = q.f;
	const bool project = q.project();
	const size_t np = tf->n, nf = f->n, nr = f->nr_cams;
	// the window form reads neither the rig (MtMcInv, cams, masks stay null) nor outlier, scales, nlevels and th; the projection form none of the last three
	t.n = tf->n; t.npoints = pts->n; t.project = project ? 1 : 0; t.nrCams = f->nr_cams; t.nlevels = f->nlevels; t.th = q.th;
	t.windowSize = (double)q.windowSize; t.minLevel = q.minLevel; t.maxLevel = q.maxLevel;
	st.in(&t.keys, tf->keys, np * sizeof(mcs_keypoint)); st.in(&t.cam, tf->cam, np * 4); st.in(&t.points, tf->points, np * 4);
	st.in(&t.outlier, project ? tf->outlier : nullptr, np);
	st.in(&t.pos, pts->pos, (size_t)pts->n * 24); st.in(&t.flags, pts->flags, (size_t)pts->n);
	st.in(&a.pdesc, tf->desc, np * tf->stride); st.in(&a.pmask, tf->mask, np * tf->stride);
	if (project) {
		st.in(&t.MtMcInv, rig->MtMc_inv, nr * 128); st.in(&t.cams, rig->cams, nr * sizeof(mcs_ocam));
		stage_mirror_masks(st, &t.masks, rig->mirror_masks, q.kind == MCS_MEM_HOST, rig->cams, f->nr_cams, maskSlots);
		st.in(&t.scales, f->scale_factors, (size_t)f->nlevels * 8);
	}
	const Thresholds th = window_thresholds(q.dim, tf->mask != nullptr);
	a.nproj = tf->n; a.pstride = tf->stride;
	a.th = 1.0; a.ratio = q.nnratio; a.dim = q.dim; a.rule = project ? (int)MCS_WINDOW_BEST : (int)MCS_WINDOW_RATIO; a.cap = kProjListK;
	a.thHigh = th.high; a.thLow = th.low;
	a.px = t.px; a.py = t.py; a.rad = t.rad; a.minLvl = t.minLvl; a.maxLvl = t.maxLvl; a.pcam = t.pcam; a.active = t.active; a.rowDiv = 0;
	stage_frame(st, a, f, project ? Assigned::Callers : Assigned::Piece, p.taken);   // vpMapPointMatches2 starts from NULLs (:333): `taken` is zeroed behind commit()
	a.match = p.matchSlot;
	st.out(&a.nmatches, q.nmatches, 4);
	tail.matchSlot = p.matchSlot; tail.n = tf->n; tail.nfeat = f->n; tail.clearDropped = project ? 1 : 0;
	st.out(&tail.matchFeat, q.matchFeat, nf * 4);
	if (q.featPoints) { if (project) st.inout(&tail.featPoints, q.featPoints, nf * 4); else st.out(&tail.featPoints, q.featPoints, nf * 4); }
}

static int tracked_launch(mcs_ctx* c, const TrackedCall& q, const TrackedPieces& p, const TrackArgs& t, const ProjArgs& a, TrackTailArgs& tail, hipStream_t s) {
	const bool project = q.project();
	const size_t nf = q.f->n;
	tail.points = t.points; tail.assigned = project ? a.assigned : nullptr; tail.removed = q.checkOrientation ? p.removed : nullptr; tail.nmatches = a.nmatches;
	if (!project) HIPCHK(hipMemsetAsync(p.taken, 0, nf, s));
	c->tic("track_probes"); launch_track_probes(t, s); c->toc("track_probes");
	// grids sized by the host-known slot count; an idle slot leaves at once (k_proj_candidates) and the greedy pass resolves it to -1
	c->tic("track_candidates"); launch_proj_candidates(a, s); c->toc("track_candidates");
	c->tic("track_greedy"); launch_proj_greedy(a, s); c->toc("track_greedy");
	c->tic("track_tail");
	HIPCHK(hipMemsetAsync(tail.matchFeat, 0xFF, nf * 4, s));
	if (!project && tail.featPoints) HIPCHK(hipMemsetAsync(tail.featPoints, 0xFF, nf * 4, s));
	launch_track_invert(tail, s);
	if (q.checkOrientation) {   // :2096-2115 variant 0, :442-462 variant 1; rot = tracked angle - frame angle: the slot is the frame's feature, so swapped
		const float* angF = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.keys) + offsetof(mcs_keypoint, angle));
		const float* angT = reinterpret_cast<const float*>(reinterpret_cast<const char*>(t.keys) + offsetof(mcs_keypoint, angle));
		launch_rotation_consistency(project ? 0 : 1, angF, (int)sizeof(mcs_keypoint), angT, (int)sizeof(mcs_keypoint), nullptr, tail.matchFeat, (int)nf, 1, p.removed, s);
	}
	launch_track_finish(tail, s);
	c->toc("track_tail");
	c->lastResultStream = s;   // every output is complete on the context's stream
	return MCS_OK;
}

static int tracked_common(mcs_ctx* c, const TrackedCall& q) {
	if (int r = guard_tracked(c, q, c && c->asyncSearch)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (q.tf->n == 0 || q.f->n == 0) return tracked_empty(c, q, s);
	if (q.kind == MCS_MEM_HOST)
		if (int r = guard_tracked_content(q)) return r;
	if (int r = ctx_join_greedy(c, s)) return r;   // the frame's arrays may come from a search whose greedy pass runs on the side stream
	TrackArgs t{};
	ProjArgs a{};
	TrackTailArgs tail{};
	TrackedPieces p;
	if (int r = tracked_layout(c, q, t, a, p)) return r;
	Staging st(c, q.kind == MCS_MEM_HOST);
	std::vector<const uint8_t*> maskSlots(q.f->nr_cams, nullptr);
	tracked_stage(st, q, p, t, a, tail, maskSlots);
	if (int r = st.commit()) return r;
	if (int r = tracked_launch(c, q, p, t, a, tail, s)) return r;
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_search_last_frame(mcs_ctx* c, const mcs_tracked_frame* last, const mcs_point_table* pts, const mcs_rig_view* rig, const mcs_frame_view* cur, double th,
                          int dim, int check_orientation, mcs_mem_kind kind, int32_t* match_cur, int32_t* cur_points, int32_t* nmatches) {
	if (!rig) return null_argument();
	return tracked_common(c, TrackedCall{last, pts, rig, cur, th, 0, 0, 0x7FFFFFFF, 1.0, dim, check_orientation, kind, match_cur, cur_points, nmatches});
}

int mcs_window_search_frames(mcs_ctx* c, const mcs_tracked_frame* f1, const mcs_point_table* pts, const mcs_frame_view* f2, int window_size, int min_level,
                             int max_level, double nnratio, int dim, int check_orientation, mcs_mem_kind kind, int32_t* match21, int32_t* points2,
                             int32_t* nmatches) {
	return tracked_common(c, TrackedCall{f1, pts, nullptr, f2, 0.0, window_size, min_level, max_level, nnratio, dim, check_orientation, kind, match21, points2, nmatches});
}
