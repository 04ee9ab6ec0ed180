// mcs_newpoints.hip — cLocalMapping::CreateNewMapPoints (src/cLocalMapping.cpp:223-381): the mapping thread's chain, keyframe in, new map points out.
//   k_np_setup        per neighbour, once: z = row 2 of MtMc_inv[cam(i)] (X, 1) of every feature that holds a map point (ComputeSceneMedianDepth,
//                     src/cMultiKeyFrame.cpp:747-778); workgroup 0 also forms the nrCams x nrCams essential matrices ComputeE(kf1.MtMc_inv[c1], kf2.MtMc[c2])
//                     (src/misc.cpp:71-85, as src/cORBmatcher.cpp:988-999 calls it) and baseline = norm(Ow2 - Ow1) (:246-248)
//   k_np_median       thread per depth: its rank among all depths; the one of rank (n - 1) / 2 is vDepths[(n - 1) / 2] of the ascending sort (a value
//                     selection: equal depths are the same double), and with it the gate baseline / median < 0.01 (:250-254)
//   k_np_triangulate  thread per feature of the current keyframe that has a match: the loop body :272-361 statement by statement (parallax, relOri,
//                     triangulate_point of src/misc.cpp:25-50, both reprojections through omni_world_to_img, the distance check); in the chain it also clears
//                     valid1[idx1] of an accepted match (AddMapPoint(pMP, idx1), :367) and the matches of a gated neighbour
//   k_np_compact      one workgroup per pair: the accepted matches in the reference's order (ascending idx1, src/cORBmatcher.cpp:1140-1152)
// mcs_create_new_map_points enqueues, per neighbour in the caller's order, the triangulation search (csrc/mcs_capi_match.hip) with the query side's valid flags read
// from a device working copy, then k_np_triangulate + k_np_compact behind the search's greedy pass (an event, no host wait); the next neighbour's search is enqueued
// behind them on the context's stream.  FP64 throughout, no contraction (-ffp-contract=off): every product and sum is the reference's, in its order; the OpenCV
// pieces are restated as DESIGN.md section 7 lists them.
#include "mcs_host.h"
#include "mcs_geom.h"
#include <algorithm>
#include <cstddef>

namespace mcs {
void launch_rotation_consistency(int variant, const float* angleSlot, int strideSlot, const float* anglePartner, int stridePartner, const int* accepted, int* match,
                                 int n, int swapped, int* removed, hipStream_t s);

struct NpKf {   // device view of one keyframe (mcs_kf_geom with every pointer on the GPU)
	const double* MtMc; const double* MtMcInv; const double* Mt; const mcs_ocam* cams;
	const double* rays; const mcs_keypoint* keys; const int* cam; int n, nrCams;
};

struct NpSetupArgs {
	NpKf k1, k2;
	const double* mpPos; const int* mpCam; int nmp;   // the neighbour's features that hold a map point: world position, camera
	double* z;                                        // [nmp] scratch
	double* E;                                        // [nrCams * nrCams][9] or nullptr (the caller's own blocks are used)
	double* baseline; double* median; uint8_t* skip;  // this neighbour's entries
};

struct NpTriArgs {
	NpKf k1, k2;
	const int* match12;     // [n1] feature of keyframe 2 matched to feature i, or -1
	int* matchClear;        // chain only: the same array, cleared for a gated neighbour
	const uint8_t* skip;    // this pair's "skipped" flag, or nullptr
	uint8_t* valid1;        // chain only: working copy of the current keyframe's "has no map point yet"
	double cosThresh, maxDist;
	int* verdict; double* x3D;
};

// cv::Matx33d ComputeE(const cv::Matx44d& T1, const cv::Matx44d& T2) (src/misc.cpp:71-85)
__device__ void np_compute_E(const double* T1, const double* T2, double* E) {
	double R12[9], N[9], t12[3];
	for (int i = 0; i < 3; ++i) {   // R1w * R2w.t() and (-R1w) * R2w.t()
		const double neg[3] = {-T1[4 * i], -T1[4 * i + 1], -T1[4 * i + 2]};
		for (int j = 0; j < 3; ++j) { R12[3 * i + j] = dot3(T1 + 4 * i, T2 + 4 * j); N[3 * i + j] = dot3(neg, T2 + 4 * j); }
	}
	const double t1w[3] = {T1[3], T1[7], T1[11]}, t2w[3] = {T2[3], T2[7], T2[11]};
	mat3_vec3(N, 3, t2w, t12);
	for (int i = 0; i < 3; ++i) t12[i] = t12[i] + t1w[i];
	const double ialpha = 1. / norm3(t12);   // Vec operator/=(double) of OpenCV 3.x: a multiplication by 1./alpha
	for (int i = 0; i < 3; ++i) t12[i] = t12[i] * ialpha;
	const double S[9] = {0.0, -t12[2], t12[1], t12[2], 0.0, -t12[0], -t12[1], t12[0], 0.0};   // Skew (include/misc.h:58-64)
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			double s = 0;
			for (int k = 0; k < 3; ++k) s += S[3 * i + k] * R12[3 * k + j];
			E[3 * i + j] = s;
		}
}

__global__ __launch_bounds__(256) void k_np_setup(NpSetupArgs a) {
	const int g = blockIdx.x * 256 + threadIdx.x;
	if (g < a.nmp) {   // src/cMultiKeyFrame.cpp:764-771
		const int c = a.mpCam[g];
		double z = __longlong_as_double(0x7FF8000000000000ll);   // a camera index outside the rig: no depth
		if (c >= 0 && c < a.k2.nrCams) {
			double r[3];
			matx44_point<3>(a.k2.MtMcInv + 16 * (size_t)c, a.mpPos + 3 * (size_t)g, r);
			z = r[2];
		}
		a.z[g] = z;
	}
	if (blockIdx.x != 0) return;
	if (a.E) {
		const int nr = a.k1.nrCams;
		for (int t = threadIdx.x; t < nr * nr; t += 256)
			np_compute_E(a.k1.MtMcInv + 16 * (size_t)(t / nr), a.k2.MtMc + 16 * (size_t)(t % nr), a.E + 9 * (size_t)t);
	}
	if (threadIdx.x == 0) {   // src/cLocalMapping.cpp:230, 246-248; GetCameraCenter = Hom2T(M_t)
		double vb[3];
		for (int k = 0; k < 3; ++k) vb[k] = a.k2.Mt[4 * k + 3] - a.k1.Mt[4 * k + 3];
		*a.baseline = norm3(vb);
		*a.median = __longlong_as_double(0x7FF8000000000000ll);   // stays NaN only when no depth has the wanted rank (a NaN depth: the reference's sort is undefined then)
		*a.skip = 0;
	}
}

__global__ __launch_bounds__(256) void k_np_median(const double* __restrict__ z, int n, const double* __restrict__ baseline, double* median, uint8_t* skip) {
	__shared__ double tile[256];
	const int j = blockIdx.x * 256 + threadIdx.x;
	const double zj = j < n ? z[j] : 0.0;
	int less = 0, leq = 0;
	for (int base = 0; base < n; base += 256) {
		__syncthreads();
		if (base + (int)threadIdx.x < n) tile[threadIdx.x] = z[base + threadIdx.x];
		__syncthreads();
		const int m = min(256, n - base);
		for (int k = 0; k < m; ++k) { const double v = tile[k]; less += v < zj; leq += v <= zj; }
	}
	const int r = (n - 1) / 2;   // vDepths[(vDepths.size() - 1) / q], q = 2
	if (j < n && less <= r && r < leq) {   // every thread that gets here holds the same double
		*median = zj;
		const double ratioBaselineDepth = *baseline / zj;
		*skip = ratioBaselineDepth < 0.01 ? 1 : 0;
	}
}

// the Vec4d overload of WorldToCamHom_fast (src/cam_system_omni.cpp:92-112); one body for both reprojections
__device__ __noinline__ bool np_world_to_cam(const NpKf& kf, int c, const double* pt4, double& u, double& v) {
	return world_to_cam_hom_fast(kf.MtMcInv + 16 * (size_t)c, ocam_dev_of(kf.cams[c]), pt4[0], pt4[1], pt4[2], u, v, pt4[3]);
}

enum { NP_NONE = 0, NP_ACCEPTED = 1, NP_PARALLAX = 2, NP_BEHIND1 = 3, NP_REPROJ1 = 4, NP_BEHIND2 = 5, NP_REPROJ2 = 6, NP_DISTANCE = 7, NP_SKIPPED = 8 };

__global__ __launch_bounds__(128) void k_np_triangulate(NpTriArgs a) {
	const int i = blockIdx.x * 128 + threadIdx.x;
	if (i >= a.k1.n) return;
	double* X = a.x3D + 3 * (size_t)i;
	X[0] = 0.0; X[1] = 0.0; X[2] = 0.0;   // cv::Vec3d x3D(0.0, 0.0, 0.0), :283
	if (a.skip && *a.skip) {   // :253-254, the neighbour changes nothing
		if (a.matchClear) a.matchClear[i] = -1;
		a.verdict[i] = NP_SKIPPED;
		return;
	}
	const int idx2 = a.match12[i];
	if (idx2 < 0 || idx2 >= a.k2.n) { a.verdict[i] = NP_NONE; return; }
	const int camIdx1 = a.k1.cam[i], camIdx2 = a.k2.cam[idx2];   // :275-276
	if (camIdx1 < 0 || camIdx1 >= a.k1.nrCams || camIdx2 < 0 || camIdx2 >= a.k2.nrCams) { a.verdict[i] = NP_NONE; return; }
	const double* Tcw1 = a.k1.MtMc + 16 * (size_t)camIdx1;      // :285-288
	const double* Tcw1inv = a.k1.MtMcInv + 16 * (size_t)camIdx1;
	const double* Tcw2 = a.k2.MtMc + 16 * (size_t)camIdx2;
	double ray1[3], ray2[3];
	for (int k = 0; k < 3; ++k) { ray1[k] = a.k1.rays[3 * (size_t)i + k]; ray2[k] = a.k2.rays[3 * (size_t)idx2 + k]; }
	double rayRot1[3], rayRot2[3];
	mat3_vec3(Tcw1, 4, ray1, rayRot1);   // :297-298
	mat3_vec3(Tcw2, 4, ray2, rayRot2);
	const double cosParallax = dot3(rayRot1, rayRot2) / (norm3(rayRot1) * norm3(rayRot2));   // :300-301
	if (cosParallax < 0 || cosParallax > a.cosThresh) { a.verdict[i] = NP_PARALLAX; return; }         // :303
	double relOri[16], R12[9], t12[3];   // relOri = Tcw1inv * Tcw2 (:306), Hom2T / Hom2R (:307-308)
	matx44_mul(Tcw1inv, Tcw2, relOri);
	for (int r = 0; r < 3; ++r) { R12[3 * r] = relOri[4 * r]; R12[3 * r + 1] = relOri[4 * r + 1]; R12[3 * r + 2] = relOri[4 * r + 2]; t12[r] = relOri[4 * r + 3]; }
	// triangulate_point(t12, R12, ray1, ray2) (src/misc.cpp:25-50)
	double f2[3];
	mat3_vec3(R12, 3, ray2, f2);
	const double b0 = dot3(t12, ray1), b1 = dot3(t12, f2);
	const double a00 = dot3(ray1, ray1), a10 = dot3(ray1, f2), a01 = -a10, a11 = -dot3(f2, f2);
	double i00 = 0.0, i01 = 0.0, i10 = 0.0, i11 = 0.0;   // Matx22d::inv(), OpenCV 3.x's closed form: a zero determinant gives the zero matrix
	double d = a00 * a11 - a01 * a10;
	if (d != 0) {
		d = 1. / d;
		i11 = a00 * d; i00 = a11 * d; i01 = -a01 * d; i10 = -a10 * d;
	}
	double l0 = 0, l1 = 0;
	l0 += i00 * b0; l0 += i01 * b1;
	l1 += i10 * b0; l1 += i11 * b1;
	double x3[3];
	for (int k = 0; k < 3; ++k) {
		const double xm = l0 * ray1[k];
		const double xn = t12[k] + l1 * f2[k];
		x3[k] = (xm + xn) / 2.0;
	}
	double x3D4[4];
	matx44_point<4>(Tcw1, x3, x3D4);   // :312-314
	X[0] = x3D4[0]; X[1] = x3D4[1]; X[2] = x3D4[2];
	double u, v;
	if (np_world_to_cam(a.k1, camIdx1, x3D4, u, v)) { a.verdict[i] = NP_BEHIND1; return; }   // :323-325
	{
		const double errX1 = u - (double)a.k1.keys[i].x, errY1 = v - (double)a.k1.keys[i].y;   // :327-330
		if (sqrt(errX1 * errX1 + errY1 * errY1) > 4.0) { a.verdict[i] = NP_REPROJ1; return; }
	}
	if (np_world_to_cam(a.k2, camIdx2, x3D4, u, v)) { a.verdict[i] = NP_BEHIND2; return; }   // :337-339
	{
		const double errX2 = u - (double)a.k2.keys[idx2].x, errY2 = v - (double)a.k2.keys[idx2].y;   // :341-344
		if (sqrt(errX2 * errX2 + errY2 * errY2) > 4.0) { a.verdict[i] = NP_REPROJ2; return; }
	}
	double normal1[3], normal2[3];   // :347-351
	for (int k = 0; k < 3; ++k) { normal1[k] = x3D4[k] - a.k1.Mt[4 * k + 3]; normal2[k] = x3D4[k] - a.k2.Mt[4 * k + 3]; }
	const double dist1 = norm3(normal1), dist2 = norm3(normal2);
	if (dist1 == 0 || dist2 == 0 || dist1 > a.maxDist || dist2 > a.maxDist) { a.verdict[i] = NP_DISTANCE; return; }   // :359-361
	a.verdict[i] = NP_ACCEPTED;
	if (a.valid1) a.valid1[i] = 0;   // mpCurrentMultiKeyFrame->AddMapPoint(pMP, idx1), :367
}

// accepted matches of one pair in ascending idx1; nmatches = the matches the loop body saw (every verdict but "no match" and "pair skipped")
__global__ __launch_bounds__(1024) void k_np_compact(const int* __restrict__ match12, const int* __restrict__ verdict, const double* __restrict__ x3D, int n1,
                                                     int* nmatches, int* accCount, int* accIdx1, int* accIdx2, double* accX) {
	__shared__ int waveAcc[16], waveM[16];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	int base = 0, mtotal = 0;
	for (int start = 0; start < n1; start += 1024) {
		const int i = start + tid;
		const int vd = i < n1 ? verdict[i] : NP_NONE;
		const bool acc = vd == NP_ACCEPTED, m = vd != NP_NONE && vd != NP_SKIPPED;
		const unsigned long long bacc = __ballot(acc), bm = __ballot(m);
		__syncthreads();
		if (lane == 0) { waveAcc[wave] = __popcll(bacc); waveM[wave] = __popcll(bm); }
		__syncthreads();
		int before = 0, total = 0;
		for (int w = 0; w < 16; ++w) { if (w < wave) before += waveAcc[w]; total += waveAcc[w]; mtotal += waveM[w]; }
		if (acc) {
			const int k = base + before + __popcll(bacc & ((1ull << lane) - 1ull));
			accIdx1[k] = i; accIdx2[k] = match12[i];
			for (int q = 0; q < 3; ++q) accX[3 * (size_t)k + q] = x3D[3 * (size_t)i + q];
		}
		base += total;
	}
	if (tid == 0) { *accCount = base; if (nmatches) *nmatches = mtotal; }
}

}  // namespace mcs
using namespace mcs;

// ------------------------------------------------------------------------------------------------ C ABI
static int np_check_geom(const mcs_kf_geom& g, bool withMp) {
	if (g.n < 0 || g.nr_cams < 1 || g.nr_cams > 32) return fail(MCS_ERR_INVALID, "keyframe: n >= 0 and 1 <= nr_cams <= 32");
	if (!g.MtMc || !g.MtMc_inv || !g.M_t || !g.cams) return fail(MCS_ERR_INVALID, "keyframe: null matrices / camera models");
	if (g.n > 0 && (!g.rays || !g.keys || !g.cam)) return fail(MCS_ERR_INVALID, "keyframe: null rays / keypoints / keypoint_to_cam");
	if (withMp) {
		// ComputeSceneMedianDepth indexes vDepths[(0 - 1) / 2] of an empty vector when the keyframe holds no map point (src/cMultiKeyFrame.cpp:777)
		if (g.n_mp < 1) return fail(MCS_ERR_INVALID, "neighbour without a map point: its median depth is undefined in the reference");
		if (!g.mp_pos || !g.mp_cam) return fail(MCS_ERR_INVALID, "neighbour: null map point positions / cameras");
	}
	return MCS_OK;
}

static NpKf np_view(const mcs_kf_geom& g) {
	NpKf k;
	k.MtMc = g.MtMc; k.MtMcInv = g.MtMc_inv; k.Mt = g.M_t; k.cams = g.cams; k.rays = g.rays; k.keys = g.keys; k.cam = g.cam; k.n = g.n; k.nrCams = g.nr_cams;
	return k;
}

static int np_check_host_geom(const mcs_kf_geom& g, bool withMp) {
	for (int c = 0; c < g.nr_cams; ++c)
		if (g.cams[c].invP_deg < 1 || g.cams[c].invP_deg > MCS_MAX_POLY) return fail(MCS_ERR_INVALID, "bad polynomial degree");
	for (int i = 0; i < g.n; ++i)
		if (g.cam[i] < 0 || g.cam[i] >= g.nr_cams) return fail(MCS_ERR_INVALID, "keypoint_to_cam outside the rig");
	if (withMp)
		for (int i = 0; i < g.n_mp; ++i)
			if (g.mp_cam[i] < 0 || g.mp_cam[i] >= g.nr_cams) return fail(MCS_ERR_INVALID, "map point camera outside the rig");
	return MCS_OK;
}
// host-kind calls: a keyframe's arrays declared on the call's staging, *d the view of the staged copies
static void np_stage_geom(Staging& st, const mcs_kf_geom& g, bool withMp, mcs_kf_geom* d) {
	*d = g;
	const size_t nc = (size_t)g.nr_cams, n = (size_t)g.n;
	st.in(&d->MtMc, g.MtMc, nc * 128); st.in(&d->MtMc_inv, g.MtMc_inv, nc * 128); st.in(&d->M_t, g.M_t, 128); st.in(&d->cams, g.cams, nc * sizeof(mcs_ocam));
	st.in(&d->rays, g.rays, n * 24); st.in(&d->keys, g.keys, n * sizeof(mcs_keypoint)); st.in(&d->cam, g.cam, n * 4);
	if (withMp) { st.in(&d->mp_pos, g.mp_pos, (size_t)g.n_mp * 24); st.in(&d->mp_cam, g.mp_cam, (size_t)g.n_mp * 4); }
	else { d->mp_pos = nullptr; d->mp_cam = nullptr; d->n_mp = 0; }
}
// ... and the per-pair outputs
static void np_stage_out(Staging& st, const mcs_newpoints_out* o, size_t rows, int nsets, mcs_newpoints_out* d) {
	st.out(&d->verdict, o->verdict, rows * 4); st.out(&d->x3D, o->x3D, rows * 24); st.out(&d->acc_count, o->acc_count, (size_t)nsets * 4);
	st.out(&d->acc_idx1, o->acc_idx1, rows * 4); st.out(&d->acc_idx2, o->acc_idx2, rows * 4); st.out(&d->acc_x3D, o->acc_x3D, rows * 24);
}

static bool np_out_ok(const mcs_newpoints_out* o) { return o && o->verdict && o->x3D && o->acc_count && o->acc_idx1 && o->acc_idx2 && o->acc_x3D; }

static void np_launch_pair(const NpTriArgs& t, int n1, int* nmatches, int* accCount, int* accIdx1, int* accIdx2, double* accX, hipStream_t s) {
	if (n1 > 0) hipLaunchKernelGGL(k_np_triangulate, dim3((n1 + 127) / 128), dim3(128), 0, s, t);
	hipLaunchKernelGGL(k_np_compact, dim3(1), dim3(1024), 0, s, t.match12, (const int*)t.verdict, (const double*)t.x3D, n1, nmatches, accCount, accIdx1, accIdx2, accX);
}

// every pointer on the device
static int np_triangulate_device(mcs_ctx* c, int nsets, const mcs_kf_geom* kf1, const mcs_kf_geom* kf2, const int32_t* match12, const uint8_t* skipped,
                                 double cosThresh, double maxDIST, const mcs_newpoints_out* out) {
	hipStream_t s = c->stream;
	if (int r = ctx_join_greedy(c, s)) return r;   // match12 may come from a search whose greedy pass runs beside
	const int n1 = kf1[0].n;
	for (int p = 0; p < nsets; ++p) {
		NpTriArgs t{};
		t.k1 = np_view(kf1[p]); t.k2 = np_view(kf2[p]);
		t.match12 = match12 + (size_t)p * n1; t.skip = skipped ? skipped + p : nullptr;
		t.cosThresh = cosThresh; t.maxDist = maxDIST;
		t.verdict = out->verdict + (size_t)p * n1; t.x3D = out->x3D + 3 * (size_t)p * n1;
		np_launch_pair(t, n1, nullptr, out->acc_count + p, out->acc_idx1 + (size_t)p * n1, out->acc_idx2 + (size_t)p * n1, out->acc_x3D + 3 * (size_t)p * n1, s);
	}
	HIPCHK(hipGetLastError());
	return MCS_OK;
}

static int np_chain_device(mcs_ctx* c, int nsets, const mcs_kf_geom* kf1, const mcs_desc_set* d1, const mcs_kf_geom* kf2, const mcs_desc_set* d2, const double* E,
                           size_t Epitch, int dim, int K, int checkOri, double cosThresh, double maxDIST, int32_t* match12, int32_t* nmatches, int32_t* fallbacks,
                           double* baseline, double* median, uint8_t* skipped, uint8_t* valid1, const mcs_newpoints_out* out) {
	hipStream_t s = c->stream;
	const int n1 = kf1->n, nr = kf1->nr_cams;
	int maxMp = 0;
	for (int p = 0; p < nsets; ++p) maxMp = std::max(maxMp, kf2[p].n_mp);
	const size_t eBlock = (size_t)nr * nr * 9;
	double* Ework = nullptr; double* z = nullptr; int* removed = nullptr; int32_t* ownFallbacks = nullptr;
	Layout lay;
	lay.piece(E ? nullptr : &Ework, E ? 0 : eBlock * 8 * nsets); lay.piece(&z, (size_t)maxMp * 8); lay.piece(&removed, 4); lay.piece(&ownFallbacks, (size_t)nsets * 4);
	HIPCHK(c->npBuf.reserve(lay.total));
	lay.place(c->npBuf.p);
	if (!fallbacks) fallbacks = ownFallbacks;
	if (int r = ctx_join_greedy(c, s)) return r;   // an earlier search's greedy pass may still read valid1
	if (n1 > 0 && valid1 != d1->valid) {
		if (d1->valid) HIPCHK(hipMemcpyAsync(valid1, d1->valid, (size_t)n1, hipMemcpyDeviceToDevice, s));
		else HIPCHK(hipMemsetAsync(valid1, 1, (size_t)n1, s));
	}
	for (int p = 0; p < nsets; ++p) {   // setup, once: the z scratch is reused in stream order
		NpSetupArgs a{};
		a.k1 = np_view(*kf1); a.k2 = np_view(kf2[p]);
		a.mpPos = kf2[p].mp_pos; a.mpCam = kf2[p].mp_cam; a.nmp = kf2[p].n_mp; a.z = z;
		a.E = Ework ? Ework + eBlock * p : nullptr;
		a.baseline = baseline + p; a.median = median + p; a.skip = skipped + p;
		const int blocks = (a.nmp + 255) / 256;
		hipLaunchKernelGGL(k_np_setup, dim3(blocks), dim3(256), 0, s, a);
		hipLaunchKernelGGL(k_np_median, dim3(blocks), dim3(256), 0, s, (const double*)z, a.nmp, (const double*)a.baseline, a.median, a.skip);
	}
	HIPCHK(hipGetLastError());
	const size_t angleOff = offsetof(mcs_keypoint, angle);
	for (int p = 0; p < nsets; ++p) {
		mcs_desc_set q = *d1;
		q.valid = valid1;   // the working copy: features that got a map point from an earlier neighbour are no longer searched (src/cORBmatcher.cpp:1017-1020)
		int32_t* m12 = match12 + (size_t)p * n1;
		const double* Ep = E ? E + Epitch * p : Ework + eBlock * p;
		// lists on the context's stream (behind the previous neighbour's k_np_triangulate), greedy pass on the side stream behind the lists
		if (int r = mcs_search_triangulation(c, 1, &q, 0, &d2[p], 0, kf1->rays, kf2[p].rays, Ep, nr, dim, K, MCS_MEM_DEVICE, m12, nmatches + p, fallbacks + p)) return r;
		if (int r = ctx_join_greedy(c, s)) return r;   // match12 is complete behind the greedy pass
		if (checkOri && n1 > 0 && kf2[p].n > 0)
			launch_rotation_consistency(3, (const float*)((const uint8_t*)kf1->keys + angleOff), (int)sizeof(mcs_keypoint),
			                            (const float*)((const uint8_t*)kf2[p].keys + angleOff), (int)sizeof(mcs_keypoint), nullptr, m12, n1, 0, removed, s);
		NpTriArgs t{};
		t.k1 = np_view(*kf1); t.k2 = np_view(kf2[p]);
		t.match12 = m12; t.matchClear = m12; t.skip = skipped + p; t.valid1 = valid1;
		t.cosThresh = cosThresh; t.maxDist = maxDIST;
		t.verdict = out->verdict + (size_t)p * n1; t.x3D = out->x3D + 3 * (size_t)p * n1;
		np_launch_pair(t, n1, nmatches + p, out->acc_count + p, out->acc_idx1 + (size_t)p * n1, out->acc_idx2 + (size_t)p * n1, out->acc_x3D + 3 * (size_t)p * n1, s);
		HIPCHK(hipGetLastError());
	}
	c->lastResultStream = s;   // every output of the chain is complete on the context's stream
	return MCS_OK;
}

extern "C" {

int mcs_triangulate_matches(mcs_ctx* c, int nsets, const mcs_kf_geom* kf1, const mcs_kf_geom* kf2, const int32_t* match12, const uint8_t* skipped,
                            double cosThresh, double maxDIST, mcs_mem_kind kind, const mcs_newpoints_out* out) {
	if (!c || !kf1 || !kf2 || !np_out_ok(out)) return fail(MCS_ERR_INVALID, "null argument");
	if (nsets < 1) return fail(MCS_ERR_INVALID, "nsets must be >= 1");
	const int n1 = kf1[0].n;
	for (int p = 0; p < nsets; ++p) {
		if (int r = np_check_geom(kf1[p], false)) return r;
		if (int r = np_check_geom(kf2[p], false)) return r;
		if (kf1[p].n != n1) return fail(MCS_ERR_INVALID, "every pair's first keyframe must have the same number of features");
	}
	if (n1 > 0 && !match12) return fail(MCS_ERR_INVALID, "null match12");
	HIPCHK(hipSetDevice(c->device));
	if (kind == MCS_MEM_DEVICE) return np_triangulate_device(c, nsets, kf1, kf2, match12, skipped, cosThresh, maxDIST, out);
	const size_t rows = (size_t)nsets * n1;
	for (int p = 0; p < nsets; ++p) {
		if (int r = np_check_host_geom(kf1[p], false)) return r;
		if (int r = np_check_host_geom(kf2[p], false)) return r;
		for (int i = 0; i < n1; ++i)
			if (match12[(size_t)p * n1 + i] >= kf2[p].n) return fail(MCS_ERR_INVALID, "match12 entry outside the second keyframe");
	}
	Staging st(c, true);
	std::vector<mcs_kf_geom> g1(nsets), g2(nsets);
	std::vector<int> same(nsets, -1);
	for (int p = 0; p < nsets; ++p) {
		// the same keyframe behind several pairs (the current keyframe of a neighbour loop) is staged once
		for (int q = 0; q < p && same[p] < 0; ++q) if (memcmp(&kf1[q], &kf1[p], sizeof(mcs_kf_geom)) == 0) same[p] = q;
		if (same[p] < 0) np_stage_geom(st, kf1[p], false, &g1[p]);
		np_stage_geom(st, kf2[p], false, &g2[p]);
	}
	const int32_t* dm = nullptr; const uint8_t* dskip = nullptr;
	st.in(&dm, match12, rows * 4); st.in(&dskip, skipped, (size_t)nsets);
	mcs_newpoints_out od{};
	np_stage_out(st, out, rows, nsets, &od);
	if (int r = st.commit()) return r;
	for (int p = 0; p < nsets; ++p) if (same[p] >= 0) g1[p] = g1[same[p]];
	return st.finish(np_triangulate_device(c, nsets, g1.data(), g2.data(), dm, dskip, cosThresh, maxDIST, &od));
}

int mcs_create_new_map_points(mcs_ctx* c, int nsets, const mcs_kf_geom* kf1, const mcs_desc_set* kf1_desc, const mcs_kf_geom* kf2, const mcs_desc_set* kf2_desc,
                              const double* E, size_t E_set_pitch, int dim, int K, int check_orientation, double cosThresh, double maxDIST, mcs_mem_kind kind,
                              int32_t* match12, int32_t* nmatches, int32_t* fallbacks, double* baseline, double* median_depth, uint8_t* skipped, uint8_t* valid1,
                              const mcs_newpoints_out* out) {
	if (!c || !kf1 || !kf1_desc || !kf2 || !kf2_desc || !np_out_ok(out)) return fail(MCS_ERR_INVALID, "null argument");
	if (nsets < 1) return fail(MCS_ERR_INVALID, "nsets must be >= 1");
	if (!nmatches || !baseline || !median_depth || !skipped) return fail(MCS_ERR_INVALID, "null output");
	if (int r = np_check_geom(*kf1, false)) return r;
	const int n1 = kf1->n, nr = kf1->nr_cams;
	if (n1 > 0 && (!match12 || !valid1)) return fail(MCS_ERR_INVALID, "null output");
	if (kf1_desc->n != n1 || kf1_desc->block_rows != 0 || (n1 > 0 && !kf1_desc->group)) return fail(MCS_ERR_INVALID, "current keyframe: descriptor set and geometry disagree (contiguous rows, group = keypoint_to_cam)");
	if (E && E_set_pitch != 0 && E_set_pitch < (size_t)nr * nr * 9) return fail(MCS_ERR_INVALID, "E_set_pitch smaller than one block of essential matrices");
	for (int p = 0; p < nsets; ++p) {   // before anything runs
		if (int r = np_check_geom(kf2[p], true)) return r;
		if (kf2[p].nr_cams != nr) return fail(MCS_ERR_INVALID, "neighbour with another number of cameras");
		if (kf2_desc[p].n != kf2[p].n || kf2_desc[p].block_rows != 0 || (kf2[p].n > 0 && !kf2_desc[p].group)) return fail(MCS_ERR_INVALID, "neighbour: descriptor set and geometry disagree (contiguous rows, group = keypoint_to_cam)");
		if (kf2_desc[p].stride != kf2_desc[0].stride || (kf2_desc[p].mask == nullptr) != (kf1_desc->mask == nullptr)) return fail(MCS_ERR_INVALID, "neighbour: descriptor stride / masks differ");
	}
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the neighbour chain runs in order: switch deferred searches off (mcs_ctx_set_async_search)");
	HIPCHK(hipSetDevice(c->device));
	if (kind == MCS_MEM_DEVICE)
		return np_chain_device(c, nsets, kf1, kf1_desc, kf2, kf2_desc, E, E_set_pitch, dim, K, check_orientation, cosThresh, maxDIST, match12, nmatches, fallbacks,
		                       baseline, median_depth, skipped, valid1, out);
	const size_t rows = (size_t)nsets * n1, eDoubles = E ? E_set_pitch * (size_t)(nsets - 1) + (size_t)nr * nr * 9 : 0;
	if (int r = np_check_host_geom(*kf1, false)) return r;
	for (int p = 0; p < nsets; ++p)
		if (int r = np_check_host_geom(kf2[p], true)) return r;
	Staging st(c, true);
	// a descriptor set whose group array is its keyframe's keypoint_to_cam shares the staged copy (bound after commit)
	auto stage_set = [&](const mcs_desc_set& d, const mcs_kf_geom& g, mcs_desc_set* o) {
		*o = d;
		const size_t n = (size_t)d.n;
		st.in(&o->desc, d.desc, n * d.stride); st.in(&o->mask, d.mask, n * d.stride); st.in(&o->valid, d.valid, n);
		if (d.group != g.cam) st.in(&o->group, d.group, n * 4);
	};
	mcs_kf_geom g1;
	mcs_desc_set s1;
	std::vector<mcs_kf_geom> g2(nsets);
	std::vector<mcs_desc_set> s2(nsets);
	np_stage_geom(st, *kf1, false, &g1);
	stage_set(*kf1_desc, *kf1, &s1);
	for (int p = 0; p < nsets; ++p) { np_stage_geom(st, kf2[p], true, &g2[p]); stage_set(kf2_desc[p], kf2[p], &s2[p]); }
	const double* dE = nullptr;
	st.in(&dE, E, eDoubles * 8);
	mcs_newpoints_out od{};
	np_stage_out(st, out, rows, nsets, &od);
	int32_t *dM = nullptr, *dN = nullptr, *dF = nullptr; double *dB = nullptr, *dMed = nullptr; uint8_t *dS = nullptr, *dV = nullptr;
	st.out(&dM, match12, rows * 4); st.out(&dN, nmatches, (size_t)nsets * 4); st.out(&dF, fallbacks, (size_t)nsets * 4); st.out(&dB, baseline, (size_t)nsets * 8);
	st.out(&dMed, median_depth, (size_t)nsets * 8); st.out(&dS, skipped, (size_t)nsets); st.out(&dV, valid1, (size_t)n1);
	if (int r = st.commit()) return r;
	if (kf1_desc->group == kf1->cam) s1.group = g1.cam;
	for (int p = 0; p < nsets; ++p) if (kf2_desc[p].group == kf2[p].cam) s2[p].group = g2[p].cam;
	// the chain's searches are device-kind calls on the staged arrays: they declare nothing on the block this call holds (a second claim would be refused)
	const int rc = np_chain_device(c, nsets, &g1, &s1, g2.data(), s2.data(), dE, E_set_pitch, dim, K, check_orientation, cosThresh, maxDIST, dM, dN, dF, dB, dMed, dS, dV, &od);
	if (rc != MCS_OK) (void)mcs_ctx_synchronize(c);   // a failed chain may leave a greedy pass on the side stream that still reads the staged arrays
	// success: every neighbour's greedy pass was joined onto the context's stream inside the chain (ctx_join_greedy after each search), so the one
	// synchronisation of that stream in finish() leaves the outputs complete and the staged arrays idle, with greedyPending already false
	return st.finish(rc);
}

}  // extern "C"
