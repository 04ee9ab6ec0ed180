// window_guard_driver.cpp — runs the argument checks of the grid-window search family (csrc/mcs_window_guard.hip) on small argument structs and prints one line
// per case: name, code, text (tab-separated).  A case calls what a host-kind entry point calls, in its order.  No HIP call; tests/test_window_guards_cpu.py.
#include "mcs_window.h"

#include <cstdio>
#include <functional>

std::string& mcs_err() { static std::string e; return e; }   // the library's is in mcs_capi.hip
using namespace mcs;

static const mcs_ctx* const CTX = reinterpret_cast<const mcs_ctx*>(0x1000);   // the checks only compare it with null

// Valid arguments of every entry point over 4 frame features, 3 probes / tracked features / map points, 2 cameras and 3 levels; a case spoils its copy.
struct Args {
	mcs_keypoint keys[4] = {};
	uint8_t desc[4 * 32] = {}, mask[4 * 32] = {}, assigned[4] = {}, flags[3] = {0, MCS_LP_SEEN, 0}, inView[6] = {1, 1, 1, 1, 1, 1}, outlier[3] = {};
	int32_t cam[4] = {0, 1, 0, 1}, width[2] = {64, 64}, height[2] = {48, 48}, level[6] = {0, 1, 2, 0, 1, 2}, points[3] = {0, -1, 2}, match[6] = {}, nm = 0, ntm = 0, vis[3] = {};
	double scales[3] = {1.0, 1.2, 1.44}, xyz[9] = {}, one[6] = {}, M[32] = {};
	float angle[4] = {};
	mcs_ocam ocam[2] = {};
	const uint8_t* mirror[2] = {desc, desc};
	mcs_frame_view f{keys, desc, nullptr, cam, assigned, 4, 32, 2, width, height, scales, 3};
	mcs_projection_set ps{one, one, one, level, cam, desc, nullptr, 3, 32};
	mcs_window_probes pr{one, one, one, level, level, cam, desc, nullptr, 3, 32, nullptr};
	mcs_local_points lp{xyz, xyz, one, one, flags, 3};
	mcs_rig_view rig{M, M, ocam, nullptr, 2};
	mcs_track_state st{inView, one, one, level, one};
	mcs_tracked_frame tf{keys, desc, nullptr, cam, points, outlier, 3, 32};
	mcs_point_table tab{xyz, flags, 3};
	int dim = 32;
	bool deferred = false;
	Args() { for (mcs_ocam& o : ocam) { o.p_deg = o.invP_deg = 5; o.width = 64; o.height = 48; } }
	void masks() { f.mask = ps.mask = pr.mask = tf.mask = mask; }

	// the entry points' host-kind check sequences
	int projection(bool host = true) { return guard_search_by_projection(CTX, &ps, &f, dim, host, match, &nm); }
	int window(mcs_window_rule rule) { return guard_window(CTX, &pr, &f, rule, dim, 0, 0, match, &nm); }
	int best(int maxDist, bool skipTaken) { return guard_window(CTX, &pr, &f, MCS_WINDOW_BEST, dim, skipTaken ? 2 : 1, maxDist, match, &nm); }
	int worldToCam(int n = 3) {
		if (int r = guard_world_to_cam(CTX, M, ocam, 2, xyz, cam, n, one, flags)) return r;
		for (const mcs_ocam& o : ocam) {
			OcamDev d;
			if (int r = ocam_to_dev(o, &d)) return r;
			if (int r = guard_image_size(o)) return r;
		}
		return MCS_OK;
	}
	LocalCall localCall(bool search) {   // the map points' descriptors are `desc`, their masks the frame's
		if (!search) return LocalCall{&lp, &rig, scales, f.nlevels, &st, nullptr, nullptr, 0, nullptr, 0.0, 0.0, 0, MCS_MEM_HOST, nullptr, nullptr, &ntm, vis};
		return LocalCall{&lp, &rig, scales, f.nlevels, &st, desc, f.mask, ps.stride, &f, 3.0, 0.8, dim, MCS_MEM_HOST, match, &nm, &ntm, vis};
	}
	int local(bool search, bool host = true) {
		const LocalCall q = localCall(search);
		if (int r = guard_local_points(CTX, q, deferred)) return r;
		return host ? guard_local_points_content(q) : MCS_OK;
	}
	TrackedCall trackedCall(bool project) { return TrackedCall{&tf, &tab, project ? &rig : nullptr, &f, 3.0, 10, 0, 0x7FFFFFFF, 0.8, dim, 1, MCS_MEM_HOST, match, match, &nm}; }
	int tracked(bool project, bool host = true) {
		const TrackedCall q = trackedCall(project);
		if (int r = guard_tracked(CTX, q, deferred)) return r;
		return host ? guard_tracked_content(q) : MCS_OK;
	}
};

static void run(const char* name, const std::function<int(Args&)>& body) {
	Args a;
	mcs_err().clear();
	const int rc = body(a);
	printf("%s\t%d\t%s\n", name, rc, rc ? mcs_err().c_str() : "");
}

int main() {
	// ---- mcs_search_by_projection
	run("projection.ok", [](Args& a) { return a.projection(); });
	run("projection.null", [](Args& a) { return guard_search_by_projection(CTX, &a.ps, &a.f, 32, true, nullptr, &a.nm); });
	run("projection.dim", [](Args& a) { a.dim = 24; return a.projection(); });
	run("projection.sizes", [](Args& a) { a.f.n = 65537; return a.projection(); });
	run("projection.nlevels", [](Args& a) { a.f.nlevels = 0; return a.projection(); });
	run("projection.masks", [](Args& a) { a.ps.mask = a.mask; return a.projection(); });
	run("projection.stride", [](Args& a) { a.ps.stride = 30; return a.projection(); });
	run("projection.level", [](Args& a) { a.level[2] = 3; return a.projection(); });
	run("projection.level_device", [](Args& a) { a.level[2] = 3; return a.projection(false); });
	run("projection.dim+sizes", [](Args& a) { a.dim = 24; a.f.n = 65537; return a.projection(); });
	run("projection.sizes+masks", [](Args& a) { a.f.n = 65537; a.ps.mask = a.mask; return a.projection(); });
	run("projection.masks+stride", [](Args& a) { a.ps.mask = a.mask; a.ps.stride = 30; return a.projection(); });
	run("projection.stride+level", [](Args& a) { a.f.stride = 30; a.level[0] = -1; return a.projection(); });
	// ---- mcs_window_match / mcs_window_best
	run("window.ok", [](Args& a) { a.masks(); return a.window(MCS_WINDOW_RATIO); });
	run("window.null", [](Args& a) { return guard_window(CTX, nullptr, &a.f, MCS_WINDOW_RATIO, 32, 0, 0, a.match, &a.nm); });
	run("window.rule", [](Args& a) { return a.window((mcs_window_rule)7); });
	run("window.rule+dim", [](Args& a) { a.dim = 0; return a.window((mcs_window_rule)0); });
	run("window.dim", [](Args& a) { a.dim = 48; return a.window(MCS_WINDOW_BEST); });
	run("window.sizes", [](Args& a) { a.f.nr_cams = 0; return a.window(MCS_WINDOW_BEST); });
	run("window.dim+sizes", [](Args& a) { a.dim = 24; a.f.n = 65537; return a.window(MCS_WINDOW_RATIO); });
	run("window.sizes+masks", [](Args& a) { a.f.n = 65537; a.f.mask = a.mask; return a.window(MCS_WINDOW_RATIO); });
	run("window.masks+stride", [](Args& a) { a.f.mask = a.mask; a.pr.stride = 30; return a.window(MCS_WINDOW_RATIO); });
	run("window.stride+assigned", [](Args& a) { a.f.stride = 34; a.f.assigned = nullptr; return a.window(MCS_WINDOW_RATIO); });
	run("window.assigned", [](Args& a) { a.f.assigned = nullptr; return a.window(MCS_WINDOW_BEST); });
	run("window.initialize_unassigned", [](Args& a) { a.f.assigned = nullptr; return a.window(MCS_WINDOW_INITIALIZE); });
	run("best.ok", [](Args& a) { return a.best(50, true); });
	run("best.max_dist", [](Args& a) { return a.best(-1, false); });
	run("best.max_dist+null", [](Args& a) { return guard_window(CTX, nullptr, &a.f, MCS_WINDOW_BEST, 32, 1, -1, a.match, &a.nm); });
	run("best.independent_unassigned", [](Args& a) { a.f.assigned = nullptr; return a.best(50, false); });
	run("best.skip_taken_unassigned", [](Args& a) { a.f.assigned = nullptr; return a.best(50, true); });
	// ---- mcs_world_to_cam / mcs_rotation_consistency
	run("world_to_cam.ok", [](Args& a) { return a.worldToCam(); });
	run("world_to_cam.null", [](Args& a) { return guard_world_to_cam(CTX, a.M, a.ocam, 2, a.xyz, a.cam, 3, nullptr, a.flags); });
	run("world_to_cam.sizes", [](Args& a) { return a.worldToCam(-1); });
	run("world_to_cam.degree", [](Args& a) { a.ocam[1].p_deg = 17; a.ocam[1].width = 0; return a.worldToCam(); });
	run("world_to_cam.image", [](Args& a) { a.ocam[1].height = 0; return a.worldToCam(); });
	run("rotation.ok", [](Args& a) { return guard_rotation_consistency(CTX, 3, a.angle, 28, a.angle, 4, a.match, 4, 4, &a.nm); });
	run("rotation.null", [](Args& a) { return guard_rotation_consistency(CTX, 0, a.angle, 28, nullptr, 28, a.match, 4, 4, &a.nm); });
	run("rotation.variant", [](Args& a) { return guard_rotation_consistency(CTX, 4, a.angle, 28, a.angle, 28, a.match, 4, 4, &a.nm); });
	run("rotation.stride", [](Args& a) { return guard_rotation_consistency(CTX, 0, a.angle, 28, a.angle, 30, a.match, 4, 4, &a.nm); });
	// ---- mcs_frustum
	run("frustum.ok", [](Args& a) { a.rig.mirror_masks = a.mirror; return a.local(false); });
	run("frustum.null", [](Args& a) { LocalCall q = a.localCall(false); q.rig = nullptr; return guard_local_points(CTX, q, false); });
	run("frustum.cams", [](Args& a) { a.rig.nr_cams = 33; return a.local(false); });
	run("frustum.nlevels", [](Args& a) { a.f.nlevels = 17; return a.local(false); });
	run("frustum.null_array", [](Args& a) { a.lp.normal = nullptr; return a.local(false); });
	run("frustum.degree", [](Args& a) { a.ocam[0].invP_deg = 0; a.ocam[0].width = 0; return a.local(false); });   // both of camera 0: the checks go camera by camera
	run("frustum.image", [](Args& a) { a.ocam[0].width = 0; a.rig.mirror_masks = a.mirror; a.mirror[0] = nullptr; return a.local(false); });
	run("frustum.mirror", [](Args& a) { a.rig.mirror_masks = a.mirror; a.mirror[1] = nullptr; return a.local(false); });
	run("frustum.degree_device", [](Args& a) { a.ocam[1].invP_deg = 0; return a.local(false, false); });
	run("frustum.empty+degree", [](Args& a) { a.lp.n = 0; a.ocam[0].invP_deg = 0; return a.local(false); });
	run("frustum.stale_level", [](Args& a) { a.level[2] = 9; return a.local(false); });   // read by the search only
	// ---- mcs_search_local_points
	run("local.ok", [](Args& a) { a.masks(); return a.local(true); });
	run("local.null_frame", [](Args&) { return null_argument(); });   // the entry point's own first statement
	run("local.null", [](Args& a) { LocalCall q = a.localCall(true); q.nmatches = nullptr; return guard_local_points(CTX, q, false); });
	run("local.cams+dim", [](Args& a) { a.rig.nr_cams = 33; a.dim = 24; return a.local(true); });
	run("local.dim", [](Args& a) { a.dim = 24; return a.local(true); });
	run("local.sizes", [](Args& a) { a.f.nr_cams = 1; return a.local(true); });
	run("local.masks", [](Args& a) { a.f.mask = a.mask; a.ps.stride = 30; LocalCall q = a.localCall(true); q.mask = nullptr; return guard_local_points(CTX, q, false); });
	run("local.stride", [](Args& a) { a.ps.stride = 30; return a.local(true); });
	run("local.deferred+stride", [](Args& a) { a.deferred = true; a.ps.stride = 30; return a.local(true); });
	run("local.deferred", [](Args& a) { a.deferred = true; return a.local(true); });
	run("local.null_array", [](Args& a) { a.f.assigned = nullptr; return a.local(true); });
	run("local.empty_null_array", [](Args& a) { a.lp.n = 0; a.f.assigned = nullptr; a.rig.cams = nullptr; return a.local(true); });
	run("local.mirror+level", [](Args& a) { a.rig.mirror_masks = a.mirror; a.mirror[0] = nullptr; a.level[2] = 9; return a.local(true); });
	run("local.level", [](Args& a) { a.level[2] = 9; return a.local(true); });             // slot [point 1][camera 0]: seen in this frame, in view
	run("local.level_unseen", [](Args& a) { a.level[0] = 9; a.level[4] = -1; return a.local(true); });   // points 0 and 2 are not stale; slots of point 1: 2, 3
	run("local.level_out_of_view", [](Args& a) { a.level[3] = 9; a.inView[3] = 0; return a.local(true); });
	run("local.level_device", [](Args& a) { a.level[2] = 9; return a.local(true, false); });
	// ---- mcs_search_last_frame
	run("last.ok", [](Args& a) { a.masks(); a.rig.mirror_masks = a.mirror; return a.tracked(true); });
	run("last.null_rig", [](Args&) { return null_argument(); });   // the entry point's own first statement
	run("last.null", [](Args& a) { TrackedCall q = a.trackedCall(true); q.pts = nullptr; return guard_tracked(CTX, q, false); });
	run("last.dim", [](Args& a) { a.dim = 8; return a.tracked(true); });
	run("last.sizes", [](Args& a) { a.tf.n = 65537; return a.tracked(true); });
	run("last.cams", [](Args& a) { a.f.nr_cams = 33; a.rig.nr_cams = 33; return a.tracked(true); });
	run("last.rig", [](Args& a) { a.f.nlevels = 17; return a.tracked(true); });
	run("last.rig+masks", [](Args& a) { a.rig.nr_cams = 3; a.tf.mask = a.mask; return a.tracked(true); });
	run("last.masks", [](Args& a) { a.tf.mask = a.mask; return a.tracked(true); });
	run("last.stride", [](Args& a) { a.tf.stride = 36; a.f.stride = 28; return a.tracked(true); });
	run("last.deferred", [](Args& a) { a.deferred = true; a.tf.keys = nullptr; return a.tracked(true); });
	run("last.null_array", [](Args& a) { a.tf.keys = nullptr; return a.tracked(true); });
	run("last.null_scales", [](Args& a) { a.f.scale_factors = nullptr; return a.tracked(true); });
	run("last.empty_null_array", [](Args& a) { a.f.n = 0; a.tf.keys = nullptr; a.rig.cams = nullptr; a.points[0] = 7; return a.tracked(true); });
	run("last.degree", [](Args& a) { a.ocam[0].invP_deg = 17; a.points[0] = 7; return a.tracked(true); });
	run("last.image", [](Args& a) { a.ocam[1].height = -1; return a.tracked(true); });
	run("last.mirror", [](Args& a) { a.rig.mirror_masks = a.mirror; a.mirror[0] = nullptr; return a.tracked(true); });
	run("last.point", [](Args& a) { a.points[2] = 3; return a.tracked(true); });
	run("last.point+camera", [](Args& a) { a.points[0] = 3; a.cam[0] = 2; return a.tracked(true); });
	run("last.camera", [](Args& a) { a.cam[2] = 2; return a.tracked(true); });
	run("last.null_point+camera", [](Args& a) { a.cam[1] = 5; return a.tracked(true); });   // points[1] = -1: nothing of this feature is read
	run("last.camera+octave", [](Args& a) { a.cam[0] = -1; a.keys[0].octave = 3; return a.tracked(true); });
	run("last.octave", [](Args& a) { a.keys[2].octave = 3; return a.tracked(true); });
	run("last.octave_device", [](Args& a) { a.keys[2].octave = 3; return a.tracked(true, false); });
	// ---- mcs_window_search_frames
	run("frames.ok", [](Args& a) { a.f.assigned = nullptr; a.f.scale_factors = nullptr; a.f.nlevels = 0; return a.tracked(false); });
	run("frames.octave", [](Args& a) { a.keys[0].octave = 9; return a.tracked(false); });   // that check is the projection form's
	run("frames.degree", [](Args& a) { a.ocam[0].invP_deg = 0; return a.tracked(false); });   // no rig is read
	run("frames.dim+sizes", [](Args& a) { a.dim = 24; a.f.n = 65537; return a.tracked(false); });
	run("frames.sizes+masks", [](Args& a) { a.f.n = 65537; a.f.mask = a.mask; return a.tracked(false); });
	run("frames.masks+stride", [](Args& a) { a.f.mask = a.mask; a.tf.stride = 30; return a.tracked(false); });
	run("frames.deferred", [](Args& a) { a.deferred = true; return a.tracked(false); });
	run("frames.point", [](Args& a) { a.points[0] = 3; return a.tracked(false); });
	run("frames.camera", [](Args& a) { a.cam[0] = 2; return a.tracked(false); });
	run("frames.null_table", [](Args& a) { a.tab.pos = nullptr; return a.tracked(false); });
	return 0;
}
