// mcs_window.h — what the entry points of the grid-window search family share (mcs_capi_window.hip, mcs_capi_track.hip): their argument checks
// (mcs_window_guard.hip: host logic only, no HIP call; tests/test_window_guards_cpu.py runs it alone), the thresholds and the staging of a frame and a rig.
#pragma once
#include "mcs_host.h"

namespace mcs {

// ---- argument checks, one function per entry point and stage.  MCS_OK, or the refusal's code with its text left for mcs_last_error().  The order of the
// checks inside a function is part of the ABI (which of two violated checks is reported); `c` is only compared with null.
int null_argument();
int guard_search_by_projection(const mcs_ctx* c, const mcs_projection_set* mp, const mcs_frame_view* f, int dim, bool hostKind, const int32_t* match,
                               const int32_t* nmatches);
// bestMode 0: mcs_window_match; else mcs_window_best (maxDist is checked, rule is MCS_WINDOW_BEST; bestMode 1 does not need frame->assigned)
int guard_window(const mcs_ctx* c, const mcs_window_probes* pr, const mcs_frame_view* f, mcs_window_rule rule, int dim, int bestMode, int maxDist,
                 const int32_t* match, const int32_t* nmatches);
int guard_world_to_cam(const mcs_ctx* c, const double* MtMcInv, const mcs_ocam* cams, int nrCams, const double* pts3, const int32_t* cam, int n, const double* uv,
                       const uint8_t* flags);
int guard_image_size(const mcs_ocam& cam);
int guard_rotation_consistency(const mcs_ctx* c, int variant, const float* angleSlot, int strideSlot, const float* anglePartner, int stridePartner,
                               const int32_t* match, int n, int nPartner, const int32_t* removed);
// the arguments of mcs_frustum (f == nullptr) / mcs_search_local_points and of mcs_window_search_frames (rig == nullptr) / mcs_search_last_frame
struct LocalCall {
	const mcs_local_points* pts; const mcs_rig_view* rig; const double* scales; int nlevels; const mcs_track_state* stt;
	const uint8_t* desc; const uint8_t* mask; int stride; const mcs_frame_view* f; double th, nnratio; int dim; mcs_mem_kind kind;
	int32_t* match; int32_t* nmatches; int32_t* nToMatch; int32_t* visibleInc;
	bool search() const { return f != nullptr; }
	size_t slots() const { return (size_t)pts->n * rig->nr_cams; }
};
struct TrackedCall {
	const mcs_tracked_frame* tf; const mcs_point_table* pts; const mcs_rig_view* rig; const mcs_frame_view* f; double th; int windowSize, minLevel, maxLevel;
	double nnratio; int dim, checkOrientation; mcs_mem_kind kind; int32_t* matchFeat; int32_t* featPoints; int32_t* nmatches;
	bool project() const { return rig != nullptr; }
};
// asyncSearch: deferred searches are on (mcs_ctx_set_async_search)
int guard_local_points(const mcs_ctx* c, const LocalCall& q, bool asyncSearch);
int guard_tracked(const mcs_ctx* c, const TrackedCall& q, bool asyncSearch);
// the scans of a host-kind call's contents: what the kernels index with (device kind: the caller's contract).  They read the arrays the checks above require
// of non-empty input only, so empty input passes unread (the entry points return before they get here).
int guard_local_points_content(const LocalCall& q);
int guard_tracked_content(const TrackedCall& q);

// TH_HIGH_ / TH_LOW_ (src/cORBmatcher.cpp:46-65)
struct Thresholds { int high, low; };
inline Thresholds window_thresholds(int dim, bool havingMasks) {
	return havingMasks ? Thresholds{(int)floor(1.5 * dim), (int)floor((double)dim)} : Thresholds{3 * dim, 2 * dim};
}

// The frame's side of the window matcher's arguments.  `assigned`: the caller's array, read and updated in place (null where the caller has none); scratch that
// the entry point zeroes behind commit(); or a piece of the entry point's own (mcs_window_search_frames: F2's own matches are neither read nor written).
enum class Assigned { Callers, Scratch, Piece };
inline void stage_frame(Staging& st, ProjArgs& a, const mcs_frame_view* f, Assigned how, uint8_t* piece = nullptr) {
	const size_t nf = f->n, nc = f->nr_cams;
	a.nfeat = f->n; a.fstride = f->stride; a.nrCams = f->nr_cams;
	st.in(&a.keys, f->keys, nf * sizeof(mcs_keypoint)); st.in(&a.fdesc, f->desc, nf * f->stride); st.in(&a.fmask, f->mask, nf * f->stride); st.in(&a.fcam, f->cam, nf * 4);
	st.in(&a.width, f->width, nc * 4); st.in(&a.height, f->height, nc * 4);
	if (how == Assigned::Callers) st.inout(&a.assigned, f->assigned, nf);
	else if (how == Assigned::Scratch) st.scratch(&a.assigned, nf);
	else a.assigned = piece;
}

// The per-camera level-0 mirror masks as the kernels read them: a table of nr device pointers in device memory, or null (bounds test alone).  A table in host
// memory (any host-kind call; mcs_world_to_cam for either kind) has every mask staged, cams[k].width x height bytes, and is uploaded: commit() binds slots[]
// before it reads the sources, so `slots` (nr entries) lives until then.  A device-kind rig's table is the caller's.
inline void stage_mirror_masks(Staging& st, const uint8_t* const** table, const uint8_t* const* masks, bool hostTable, const mcs_ocam* cams, int nr,
                               std::vector<const uint8_t*>& slots) {
	if (!masks || !hostTable) { *table = masks; return; }
	for (int k = 0; k < nr; ++k) st.in(&slots[k], masks[k], (size_t)cams[k].width * cams[k].height);
	st.upload(table, slots.data(), sizeof(void*) * nr);
}

}  // namespace mcs
