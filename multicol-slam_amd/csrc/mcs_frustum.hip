// mcs_frustum.hip — the search step of cTracking::TrackLocalMap without a host visit:
//   bool cMultiFrame::isInFrustum(int cam, cMapPoint*, double viewingCosLimit)     src/cMultiFrame.cpp:218-270
//   the frustum loop and the gate of cTracking::SearchReferencePointsInFrustum   src/cTracking.cpp:978-1011
// One thread per (map point i, camera c) slot p = i * nrCams + c, which is the visiting order of cORBmatcher::SearchByProjection(F, mapPoints, th)
// (src/cORBmatcher.cpp:75-85: map point, then camera).  The search therefore runs on the slots as they lie (mcs_project.hip: ProjArgs.active / rowDiv):
// nothing is compacted and no count leaves the device.  FP64, no contraction; the statements are the reference's, its quirks included.
#include "mcs_geom.h"

namespace mcs {

// std::lower_bound(mvScaleFactors.begin(), mvScaleFactors.end(), ratio) - begin(): libstdc++'s bisection, so that a NaN ratio (every comparison false) ends at
// begin() and an infinite one at end(), whatever the factors are
__device__ __forceinline__ int lower_bound_index(const double* s, int n, double v) {
	int first = 0, len = n;
	while (len > 0) {
		const int half = len >> 1, mid = first + half;
		if (s[mid] < v) { first = mid + 1; len = len - half - 1; }
		else len = half;
	}
	return first;
}

__global__ __launch_bounds__(256) void k_frustum(FrustumArgs a) {
	const int p = blockIdx.x * 256 + threadIdx.x;
	const int nslots = a.npoints * a.nrCams;
	const bool live = p < nslots;
	const int i = live ? p / a.nrCams : 0, c = live ? p - i * a.nrCams : 0;
	bool inView = false;
	if (live) {
		if (a.pcam) a.pcam[p] = c;
		// :985-988: a point seen in this frame or bad is not projected; its slots keep whatever earlier frames left there.  Bits 0 and 1 alone have a meaning
		if ((a.flags[i] & (MCS_LP_BAD | MCS_LP_SEEN)) == 0) {
			const double P0 = a.pos[3 * (size_t)i], P1 = a.pos[3 * (size_t)i + 1], P2 = a.pos[3 * (size_t)i + 2];
			const mcs_ocam& m = a.cams[c];
			double u, v;
			(void)world_to_cam_hom_fast(a.MtMcInv + 16 * (size_t)c, ocam_dev_of(m), P0, P1, P2, u, v);   // the bool it returns (ptRot.z <= 0) is ignored, :228
			if (in_mirror_mask(u, v, m.width, m.height, a.masks ? a.masks[c] : nullptr)) {   // :230
				const double* T = a.MtMc + 16 * (size_t)c;
				const double PO[3] = {P0 - T[3], P1 - T[7], P2 - T[11]};                         // :238
				const double dist = norm3(PO);                                                   // :239
				const double minD = a.minDist[i], maxD = a.maxDist[i];
				if (!(dist < minD || dist > maxD)) {                                             // :241 (a NaN passes)
					const double viewCos = dot3(PO, a.normal + 3 * (size_t)i) / dist;            // :247; viewingCosLimit is never applied (:249-250)
					const double ratio = dist / minD;                                            // :253
					int lvl = lower_bound_index(a.scales, a.nlevels, ratio);                     // :255-257
					if (lvl >= a.nlevels) lvl = a.nlevels - 1;                                   // :259-260
					a.projX[p] = u; a.projY[p] = v; a.level[p] = lvl; a.viewCos[p] = viewCos;    // :264-267
					inView = true;
				}
			}
			a.inView[p] = inView ? 1 : 0;   // :220 / :263; a rejected slot keeps its other four fields
		}
		a.fresh[p] = inView ? 1 : 0;
	}
	const unsigned long long b = __ballot(inView);
	if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.nToMatch, __popcll(b));   // ++nToMatch, :996 (integers: any order gives the same sum)
}

// per map point: IncreaseVisible() once per camera that came into view (:995), and which of its slots SearchByProjection visits:
// mbTrackInView[cam] (fresh or stale) of a point that is not bad (src/cORBmatcher.cpp:79-85), and only if nToMatch > 0 (:1001)
__global__ __launch_bounds__(256) void k_frustum_finish(FrustumArgs a) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= a.npoints) return;
	const bool search = *a.nToMatch > 0 && !(a.flags[i] & MCS_LP_BAD);
	int vis = 0;
	for (int c = 0; c < a.nrCams; ++c) {
		const size_t p = (size_t)i * a.nrCams + c;
		vis += a.fresh[p];
		// a stale slot's level is the caller's: outside [0, nlevels) it would index mvScaleFactors out of bounds in the reference, here it is not searched
		if (a.active) a.active[p] = (search && a.inView[p] && (unsigned)a.level[p] < (unsigned)a.nlevels) ? 1 : 0;
	}
	a.visibleInc[i] = vis;
}

void launch_frustum(const FrustumArgs& a, hipStream_t s) {
	(void)hipMemsetAsync(a.nToMatch, 0, sizeof(int), s);
	if (a.npoints <= 0) return;
	const int nslots = a.npoints * a.nrCams;
	hipLaunchKernelGGL(k_frustum, dim3((nslots + 255) / 256), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_frustum_finish, dim3((a.npoints + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace mcs
