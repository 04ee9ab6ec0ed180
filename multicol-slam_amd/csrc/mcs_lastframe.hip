// mcs_lastframe.hip — the frame-to-frame searches of the tracker without a host visit:
//   int cORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th)                      src/cORBmatcher.cpp:1990-2118   (cTracking::TrackWithMotionModel)
//   int cORBmatcher::WindowSearch(F1, F2, windowSize, vpMapPointMatches2, minLvl, maxLvl) src/cORBmatcher.cpp:326-473     (cTracking::TrackPreviousFrame)
// One slot per feature of the tracked frame, in feature order, which is the reference's visiting order.  k_track_probes decides which slots the reference
// would search and writes their windows; the window matcher of mcs_project.hip then runs on the slots as they lie (ProjArgs.active), as it does for the
// local map (mcs_frustum.hip): nothing is compacted and no count leaves the device.  The tail turns feature-per-slot into slot-per-feature, which is what
// the rotation filter and the caller read.  FP64, no contraction; the projection is mcs_geom.h's world_to_cam_hom_fast.
#include "mcs_geom.h"

namespace mcs {

__global__ __launch_bounds__(256) void k_track_probes(TrackArgs t) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= t.n) return;
	const int id = t.points[i];                      // mvpMapPoints[i]: -1 is NULL (:2007, :348)
	const int c = t.cam[i];
	const mcs_keypoint kp = t.keys[i];
	bool act = false;
	// an id outside the tables or a camera outside the rig would index out of bounds: such a slot is idle (the host-kind call refuses it beforehand)
	if (id >= 0 && id < t.npoints && (unsigned)c < (unsigned)t.nrCams && !(t.flags[id] & 1)) {   // isBad(), :2009, :351
		if (t.project) {
			if (!(t.outlier && t.outlier[i]) && (unsigned)kp.octave < (unsigned)t.nlevels) {     // :2014; the octave indexes mvScaleFactors (:2028)
				const double P0 = t.pos[3 * (size_t)id], P1 = t.pos[3 * (size_t)id + 1], P2 = t.pos[3 * (size_t)id + 2];
				const mcs_ocam& m = t.cams[c];
				double u, v;
				(void)world_to_cam_hom_fast(t.MtMcInv + 16 * (size_t)c, ocam_dev_of(m), P0, P1, P2, u, v);   // the bool it returns (ptRot.z <= 0) is ignored, :2020
				if (in_mirror_mask(u, v, m.width, m.height, t.masks ? t.masks[c] : nullptr)) {   // :2022
					t.px[i] = u; t.py[i] = v;
					t.rad[i] = t.th * t.scales[kp.octave];                                   // :2028
					t.minLvl[i] = kp.octave - 1; t.maxLvl[i] = kp.octave + 1;                // :2032; octave 0 gives [-1, 1], a checked range
					act = true;
				}
			}
		} else {
			const bool bMinLevel = t.minLevel > 0, bMaxLevel = t.maxLevel < 0x7FFFFFFF;         // :341-342
			if (!(bMinLevel && kp.octave < t.minLevel) && !(bMaxLevel && kp.octave > t.maxLevel)) {   // :357-363
				t.px[i] = (double)kp.x; t.py[i] = (double)kp.y; t.rad[i] = t.windowSize;     // :367-368
				t.minLvl[i] = -1; t.maxLvl[i] = -1;                                          // GetFeaturesInArea's defaults: no level check
				act = true;
			}
		}
	}
	t.pcam[i] = (unsigned)c < (unsigned)t.nrCams ? c : 0;
	t.active[i] = act ? 1 : 0;
}

// matchFeat holds -1 everywhere (memset) on entry; a feature is taken by at most one slot, so no two threads write the same entry
__global__ __launch_bounds__(256) void k_track_invert(TrackTailArgs t) {
	const int p = blockIdx.x * 256 + threadIdx.x;
	if (p >= t.n) return;
	const int j = t.matchSlot[p];
	if (j >= 0 && j < t.nfeat) t.matchFeat[j] = p;
}

// after the rotation filter: a slot whose feature no longer points back at it lost its match (:2104-2114, :450-461)
__global__ __launch_bounds__(256) void k_track_finish(TrackTailArgs t) {
	const int p = blockIdx.x * 256 + threadIdx.x;
	if (p == 0 && t.removed) *t.nmatches -= *t.removed;   // --nmatches per dropped match
	if (p >= t.n) return;
	const int j = t.matchSlot[p];
	if (j < 0 || j >= t.nfeat) return;
	if (t.matchFeat[j] == p) {
		if (t.featPoints) t.featPoints[j] = t.points[p];   // CurrentFrame.mvpMapPoints[bestIdx2] = pMP, :2075 / vpMapPointMatches2[bestIdx2] = pMP1, :428
	} else {
		if (t.assigned) t.assigned[j] = 0;                 // CurrentFrame.mvpMapPoints[...] = NULL, :2110
		if (t.featPoints && t.clearDropped) t.featPoints[j] = -1;
	}
}

void launch_track_probes(const TrackArgs& t, hipStream_t s) {
	if (t.n > 0) hipLaunchKernelGGL(k_track_probes, dim3((t.n + 255) / 256), dim3(256), 0, s, t);
}
void launch_track_invert(const TrackTailArgs& t, hipStream_t s) {
	if (t.n > 0) hipLaunchKernelGGL(k_track_invert, dim3((t.n + 255) / 256), dim3(256), 0, s, t);
}
void launch_track_finish(const TrackTailArgs& t, hipStream_t s) {
	if (t.n > 0) hipLaunchKernelGGL(k_track_finish, dim3((t.n + 255) / 256), dim3(256), 0, s, t);
}

}  // namespace mcs
