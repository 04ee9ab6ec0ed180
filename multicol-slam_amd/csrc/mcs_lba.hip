// mcs_lba.hip — cOptimizer::LocalBundleAdjustment (src/cOptimizer.cpp:461-874) as one problem over the whole device, and the entry point
// mcs_local_bundle_adjustment (include/mcs_c.h).  DESIGN.md 4n; the statement-by-statement restatement the kernels are held to is tests/lba_model.py.
// The Levenberg-Marquardt steps, the Huber pair, the wave sums and the ordered lists are csrc/mcs_lm.h's, the matrices, the camera and the derivatives
// csrc/mcs_geom.h's.
//
// The phases are separate launches on the context's stream — no grid-wide barrier, no workgroup waits for another inside a launch:
//   k_lba_prepare      per point: its edge range, the guards, the point of every edge, the level of every edge
//   k_lba_kf_lists     per free keyframe: its edges in ascending order (count, then fill), once per call
//   k_lba_rigs         per (keyframe, camera): invMat(Mt Mc) and, for a build, the factors Rc^T (dRt/dc_i)^T
//   k_lba_linearise    one wave per point, lanes over its edges: residual, Huber weight, [Build] both Jacobians per edge, Hll, b_l and the robust chi2 per point
//   k_lba_reduce       one workgroup: the chi2 over the points in a fixed order, the largest |Hll_jj|, the landmark part of computeScale
//   k_lba_pose_blocks  one workgroup per free keyframe: Hpp and b_p over its edges in ascending order
//   k_lba_iter_begin   one thread: currentChi, the screen of the first evaluation, computeLambdaInit
//   k_lba_dinv         per point: (Hll + lambda I)^-1 by Eigen's closed form, and Dinv b_l
//   k_lba_schur        one wave per block (i, j >= i) of S: walks keyframe i's edges, lanes over them, subtracts W_ip Dinv_p W_jp^T; the diagonal wave also b_s
//   k_lba_solve        one workgroup: unpivoted LDL^T of S in scratch, x_p, the failure flag
//   k_lba_apply        x_l = Dinv (b_l - W^T x_p) per point, the trial estimates of poses and points, the point's share of computeScale
//   k_lba_decide       one thread: rho, lambda / ni, accept or restore, the trial count, solve()'s return, the terminate action; the 64-byte record
//   k_lba_accept       the trial estimates become the estimates (discardTop) where the trial was accepted
//   k_lba_outlier      per point, sequential over its edges: one pass at chi2 > thHuber^2 with the point's bad flag shielding what lies behind an erasure
//   k_lba_writeback    the outputs
// Every decision that depends on arithmetic is taken on the device; the host loop reads the record after ONE stream synchronisation per trial and chooses
// between "another trial", "next iteration", "round over".  Sums: per point in lane order then a fixed shuffle tree; per keyframe thread-strided in ascending
// edge order then the same tree and the waves in order; nothing depends on the grid or the run.  No floating-point atomic (the integer ones count).
//
// The Jacobians are derived by the chain rule (the reference's generated text is not used): p = (Rt Rc)^T (X - t) - Rc^T tc, so dp/dX = (Rt Rc)^T = -dp/dt,
// which is the rotation block of invMat(Mt Mc), and dp/dc_i = Rc^T (dRt/dc_i)^T (X - t); d(u, v)/dp differentiates WorldToImg; e = z - (u, v).
#include "mcs_lba.h"
#include "mcs_geom.h"
#include "mcs_lm.h"

using namespace mcs;

namespace {

enum { PT_WRITTEN = 0, PT_KEPT = 1, PT_BAD = 2 };
constexpr int kRigDoubles = 16 + 27;   // inv (4x4), then A_i = Rc^T (dRt/dc_i)^T, i = 0..2
constexpr int kEdgeDoubles = 12 + 6 + 2 + 1;   // Jp [2][6], Jl [2][3], e [2], rho[1] * information

struct LbaCtl {   // the Levenberg-Marquardt state, on the device
	LmState lm;
	double sumChi, maxDiag, sumScale;   // of k_lba_reduce
	int nonfinite, solveOk, accepted, nActive, nErased[2];
};
struct LbaRecord {   // 64 bytes, page-locked host memory: what the host loop reads
	int more, resultOk, why, gainStop, qmax, nonfinite, nActive, accepted;
	double lambda, chi2;
	int nErased[2], pad[2];
};
static_assert(sizeof(LbaRecord) == 64, "the control record is 64 bytes");

struct LbaDev {
	int nKfs, nLocal, nPoints, nEdges, nrCams, nlevels, nFree;
	double delta, dsqr;
	// the caller's arrays (or their staged copies)
	double* kfPoseIO; double* kfT; double* posIO; const int* ptFirst; const int* edgeKf; const int* edgeCam; const mcs_keypoint* key;
	const int* totalObs; const int* badObs; const double* McMin; const mcs_ocam* cams; const double* invSigma2; uint8_t* edgeStateOut; uint8_t* ptStateOut;
	// scratch
	const int* fidx; const int* freeKf;           // [nKfs] free index or -1, [nFree] keyframe of a free index
	OcamDev* cam; double* dInvP; double* McH;     // [nr], [nr][MCS_MAX_POLY], [nr][16]
	double* pose; double* poseT; double* pos; double* posT;   // the estimates and the trial estimates
	double* rig;                                  // [nKfs * nr][kRigDoubles]
	int* ept; uint8_t* level; uint8_t* act; uint8_t* state;   // per edge: its point, its level, active in the current system, the pass that erased it
	double* edge; double* eChi;                   // [nEdges][kEdgeDoubles], [nEdges] plain chi2 of the latest evaluation
	double* Hll; double* bl; double* ptChi; double* Dinv; double* db; double* xl; double* ptScale;   // per point: 6, 3, 1, 9, 3, 3, 1
	int* ptAct; int* ptDeg; int* ptTotal; uint8_t* ptBad;
	double* Hpp; double* bp; double* xp;          // [nFree][21], [nFree][6], [6 nFree]
	int* kfCount; int* kfOff; int* kfList;        // [nFree], [nFree + 1], [nEdges]
	double* S; double* bs;                        // [6 nFree][6 nFree], [6 nFree]
	LbaCtl* ctl; LbaRecord* rec;
};

__device__ __forceinline__ bool point_range(const LbaDev& d, int p, int& a, int& b) {
	a = d.ptFirst[p]; b = d.ptFirst[p + 1];
	if (a < 0 || a > b || b > d.nEdges) { a = b = 0; return false; }
	return true;
}

// ---------------------------------------------------------------------------------------------- once per call
__global__ void k_lba_cams(LbaDev d) {
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= d.nrCams) return;
	const mcs_ocam& m = d.cams[c];
	const OcamDev o = ocam_dev_of(m);
	d.cam[c] = o;
	ocam_dinvp(m, o, d.dInvP + c * MCS_MAX_POLY);
	cayley2hom(d.McMin + 6 * c, d.McH + 16 * c);
}

__global__ void k_lba_prepare(LbaDev d) {   // d.level was set to 1 everywhere, d.ept to -1
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= d.nPoints) return;
	int a, b, n = 0;
	point_range(d, p, a, b);
	for (int e = a; e < b; ++e) {
		d.ept[e] = p;
		const int kf = d.edgeKf[e], c = d.edgeCam[e], oct = d.key[e].octave;
		if (kf < 0 || kf >= d.nKfs || c < 0 || c >= d.nrCams || oct < 0 || oct >= d.nlevels) continue;
		d.level[e] = 0;
		++n;
	}
	d.ptDeg[p] = n;
	d.ptTotal[p] = d.totalObs ? d.totalObs[p] : n;
	d.ptBad[p] = 0;
	if (n) atomicAdd(&d.ctl->nActive, n);
}

// the edges of free keyframe blockIdx.x in ascending order: Fill = false counts, Fill = true writes behind kfOff
template <bool Fill>
__global__ void __launch_bounds__(256) k_lba_kf_lists(LbaDev d) {
	const int f = blockIdx.x, kf = d.freeKf[f];
	const int n = compact_indices<Fill, 256>(d.nEdges, [&](int e) { return d.edgeKf[e] == kf; }, Fill ? d.kfList + d.kfOff[f] : nullptr);
	if (!Fill && threadIdx.x == 0) d.kfCount[f] = n;
}

__global__ void k_lba_kf_offsets(LbaDev d) {
	if (blockIdx.x || threadIdx.x) return;
	list_offsets(d.kfCount, d.kfOff, d.nFree);
}

// ---------------------------------------------------------------------------------------------- an evaluation
// invMat(Mt Mc) of every (keyframe, camera) at `poses` (EdgeProjectXYZ2MCS::computeError); build: also A_i.  freeOnly: a fixed keyframe's were computed before.
__global__ void k_lba_rigs(LbaDev d, const double* poses, int build, int freeOnly) {
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= d.nKfs * d.nrCams) return;
	const int kf = t / d.nrCams, c = t - kf * d.nrCams;
	if (freeOnly && d.fidx[kf] < 0) return;
	const double* pose = poses + 6 * kf;
	double* out = d.rig + (size_t)t * kRigDoubles;
	double Mt[16], Mct[16], inv[16];
	const double* McH = d.McH + 16 * c;
	cayley2hom(pose, Mt);
	matx44_mul(Mt, McH, Mct);
	inv_mat(Mct, inv);
	for (int k = 0; k < 16; ++k) out[k] = inv[k];
	if (!build) return;
	cayley_rot_factors(pose, Mt, McH, out + 16);
}

// One wave per point, lanes over its edges (looping above 64).  The active edges are those at level 0.  Writes the plain chi2 of every edge of the point and
// the point's robust chi2; Build: also each active edge's Jacobians, error and robust weight, the point's Hll (upper triangle) and b_l, and who is active.
template <bool Build>
__global__ void __launch_bounds__(256) k_lba_linearise(LbaDev d, const double* poses, const double* pos) {
	const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (p >= d.nPoints) return;   // the whole wave
	int a, b;
	point_range(d, p, a, b);
	const double X[3] = {pos[3 * (size_t)p], pos[3 * (size_t)p + 1], pos[3 * (size_t)p + 2]};
	double acc[10];
#pragma unroll
	for (int k = 0; k < 10; ++k) acc[k] = 0.0;
	int nact = 0;
	bool bad = false;
	for (int base = a; base < b; base += 64) {
		const int e = base + lane;
		if (e >= b) continue;
		if (d.level[e] != 0) { d.eChi[e] = 0.0; if (Build) d.act[e] = 0; continue; }
		const int kf = d.edgeKf[e], c = d.edgeCam[e];
		const double* R = d.rig + ((size_t)kf * d.nrCams + c) * kRigDoubles;
		const OcamDev& cam = d.cam[c];
		double pc[3], u, v;
		matx44_point<3>(R, X, pc);
		omni_world_to_img(cam, pc[0], pc[1], pc[2], u, v);
		const double e0 = (double)d.key[e].x - u, e1 = (double)d.key[e].y - v;
		const double w = d.invSigma2[d.key[e].octave];
		const double c2 = e0 * (w * e0) + e1 * (w * e1);   // _error.dot(information() * _error)
		double rho0, rho1;
		huber_robustify(c2, d.delta, d.dsqr, rho0, rho1);
		d.eChi[e] = c2;
		acc[9] += rho0;
		if constexpr (Build) {
			double D[2][3], Jp[2][6], Jl[2][3];
			d_world_to_img(cam, d.dInvP + c * MCS_MAX_POLY, pc[0], pc[1], pc[2], D);
			const double* pose = poses + 6 * kf;
			const double dd[3] = {X[0] - pose[3], X[1] - pose[4], X[2] - pose[5]};
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				Jl[0][k] = -(D[0][0] * R[k] + D[0][1] * R[4 + k] + D[0][2] * R[8 + k]);
				Jl[1][k] = -(D[1][0] * R[k] + D[1][1] * R[4 + k] + D[1][2] * R[8 + k]);
				const double* A = R + 16 + 9 * k;
				double dp[3];
#pragma unroll
				for (int r = 0; r < 3; ++r) dp[r] = A[3 * r] * dd[0] + A[3 * r + 1] * dd[1] + A[3 * r + 2] * dd[2];
				Jp[0][k] = -(D[0][0] * dp[0] + D[0][1] * dp[1] + D[0][2] * dp[2]);
				Jp[1][k] = -(D[1][0] * dp[0] + D[1][1] * dp[1] + D[1][2] * dp[2]);
				Jp[0][3 + k] = -Jl[0][k];
				Jp[1][3 + k] = -Jl[1][k];
			}
			const double rw = rho1 * w;   // robustInformation = rho[1] * information; no second-order term
			double* o = d.edge + (size_t)e * kEdgeDoubles;
#pragma unroll
			for (int k = 0; k < 6; ++k) { o[k] = Jp[0][k]; o[6 + k] = Jp[1][k]; bad |= !finite_(Jp[0][k]) || !finite_(Jp[1][k]); }
#pragma unroll
			for (int k = 0; k < 3; ++k) { o[12 + k] = Jl[0][k]; o[15 + k] = Jl[1][k]; bad |= !finite_(Jl[0][k]) || !finite_(Jl[1][k]); }
			o[18] = e0; o[19] = e1; o[20] = rw;
			bad |= !finite_(e0) || !finite_(e1) || !finite_(w);
			d.act[e] = 1;
			++nact;
			int s = 0;
#pragma unroll
			for (int r = 0; r < 3; ++r)
#pragma unroll
				for (int q = r; q < 3; ++q) acc[s++] += rw * (Jl[0][r] * Jl[0][q] + Jl[1][r] * Jl[1][q]);
#pragma unroll
			for (int r = 0; r < 3; ++r) acc[6 + r] += -rw * (Jl[0][r] * e0 + Jl[1][r] * e1);
		}
	}
	if (Build) {
		if (bad) atomicOr(&d.ctl->nonfinite, 1);
		wave_sum<10>(acc);
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) nact += __shfl_down(nact, off, 64);
		if (lane == 0) {
			for (int k = 0; k < 6; ++k) d.Hll[6 * (size_t)p + k] = acc[k];
			for (int k = 0; k < 3; ++k) d.bl[3 * (size_t)p + k] = acc[6 + k];
			d.ptChi[p] = acc[9];
			d.ptAct[p] = nact;
		}
	} else {
		wave_sum<1>(acc + 9);
		if (lane == 0) d.ptChi[p] = acc[9];
	}
}

// one workgroup: sum of ptChi (and, trial, of ptScale) over the points, thread-strided in ascending order, then the shuffle tree and the waves in order;
// build: the largest |Hll_jj| and the finiteness of Hll and b_l
__global__ void __launch_bounds__(1024) k_lba_reduce(LbaDev d, int build) {
	__shared__ double red[16][3];
	__shared__ int nf;
	if (threadIdx.x == 0) nf = 0;
	__syncthreads();
	double acc[2] = {0.0, 0.0}, mx = 0.0;
	bool bad = false;
	for (int p = threadIdx.x; p < d.nPoints; p += 1024) {
		acc[0] += d.ptChi[p];
		if (build) {
			const double* H = d.Hll + 6 * (size_t)p;
			mx = fmax(fmax(fabs(H[0]), fabs(H[3])), fmax(fabs(H[5]), mx));
			for (int k = 0; k < 6; ++k) bad |= !finite_(H[k]);
			for (int k = 0; k < 3; ++k) bad |= !finite_(d.bl[3 * (size_t)p + k]);
		} else if (d.ptAct[p]) acc[1] += d.ptScale[p];
	}
	if (bad) atomicOr(&nf, 1);
	wave_sum<2>(acc);
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_down(mx, off, 64));
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (lane == 0) { red[wave][0] = acc[0]; red[wave][1] = acc[1]; red[wave][2] = mx; }
	__syncthreads();
	if (threadIdx.x == 0) {
		double s0 = red[0][0], s1 = red[0][1], m = red[0][2];
		for (int w = 1; w < 16; ++w) { s0 += red[w][0]; s1 += red[w][1]; m = fmax(m, red[w][2]); }
		d.ctl->sumChi = s0;
		if (build) { d.ctl->maxDiag = m; if (nf) d.ctl->nonfinite = 1; }
		else d.ctl->sumScale = s1;
	}
}

// one workgroup per free keyframe: Hpp (upper triangle, row-major) and b_p over its active edges, thread-strided in ascending edge order
__global__ void __launch_bounds__(256) k_lba_pose_blocks(LbaDev d) {
	__shared__ double red[4][27];
	const int f = blockIdx.x, n = d.kfCount[f];
	const int* list = d.kfList + d.kfOff[f];
	double acc[27];
#pragma unroll
	for (int k = 0; k < 27; ++k) acc[k] = 0.0;
	for (int t = threadIdx.x; t < n; t += 256) {
		const int e = list[t];
		if (!d.act[e]) continue;
		const double* o = d.edge + (size_t)e * kEdgeDoubles;
		const double rw = o[20], e0 = o[18], e1 = o[19];
		int s = 0;
#pragma unroll
		for (int r = 0; r < 6; ++r)
#pragma unroll
			for (int q = r; q < 6; ++q) acc[s++] += rw * (o[r] * o[q] + o[6 + r] * o[6 + q]);
#pragma unroll
		for (int r = 0; r < 6; ++r) acc[21 + r] += -rw * (o[r] * e0 + o[6 + r] * e1);
	}
	wave_sum<27>(acc);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (lane == 0) for (int k = 0; k < 27; ++k) red[wave][k] = acc[k];
	__syncthreads();
	if (threadIdx.x < 27) {
		double t = red[0][threadIdx.x];
		for (int w = 1; w < 4; ++w) t += red[w][threadIdx.x];
		if (threadIdx.x < 21) d.Hpp[21 * f + threadIdx.x] = t; else d.bp[6 * f + threadIdx.x - 21] = t;
	}
}

__global__ void k_lba_iter_begin(LbaDev d, int first, int it) {
	if (blockIdx.x || threadIdx.x) return;
	LbaCtl& c = *d.ctl;
	lm_iter_begin(c.lm, c.sumChi);
	if (first) {   // the screen of the first evaluation: every edge's residual, Jacobians and weight (k_lba_linearise), the Huber pair, the sums
		bool nf = c.nonfinite || !finite_(d.delta) || !finite_(d.dsqr) || !finite_(c.sumChi);
		for (int k = 0; k < 21 * d.nFree; ++k) nf |= !finite_(d.Hpp[k]);
		for (int k = 0; k < 6 * d.nFree; ++k) nf |= !finite_(d.bp[k]);
		c.nonfinite = nf;
	}
	if (it == 0) {   // computeLambdaInit: tau * max |H_jj| over poses AND points
		double m = c.maxDiag;
		for (int f = 0; f < d.nFree; ++f) m = max_abs_diag<6>(d.Hpp + 21 * f, m);
		lm_start(c.lm, lm_lambda_init(m));
	}
}

// ---------------------------------------------------------------------------------------------- a trial
// Dinv = (Hll + lambda I)^-1 by Eigen's closed form (Eigen/src/LU/Inverse.h:117-158) and Dinv b_l, of every point that holds an active edge
__global__ void k_lba_dinv(LbaDev d) {
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= d.nPoints || !d.ptAct[p]) return;
	const double* H = d.Hll + 6 * (size_t)p;
	const double lam = d.ctl->lm.lambda;
	const double M[3][3] = {{H[0] + lam, H[1], H[2]}, {H[1], H[3] + lam, H[4]}, {H[2], H[4], H[5] + lam}};
	double cof[3][3];
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
			cof[i][j] = M[i1][j1] * M[i2][j2] - M[i1][j2] * M[i2][j1];
		}
	const double det = (cof[0][0] * M[0][0] + cof[1][0] * M[1][0]) + cof[2][0] * M[2][0];
	const double invdet = 1.0 / det;
	double* Di = d.Dinv + 9 * (size_t)p;
	for (int j = 0; j < 3; ++j)
		for (int i = 0; i < 3; ++i) Di[3 * j + i] = cof[i][j] * invdet;
	const double* b = d.bl + 3 * (size_t)p;
	for (int r = 0; r < 3; ++r) d.db[3 * (size_t)p + r] = (Di[3 * r] * b[0] + Di[3 * r + 1] * b[1]) + Di[3 * r + 2] * b[2];
}

__device__ __forceinline__ void add_w(const double* o, double W[6][3]) {   // W += rw * Jp^T Jl of one edge
	const double rw = o[20];
#pragma unroll
	for (int r = 0; r < 6; ++r)
#pragma unroll
		for (int a = 0; a < 3; ++a) W[r][a] += rw * (o[r] * o[12 + a] + o[6 + r] * o[15 + a]);
}

// One wave per block (i, j >= i) of S = Hpp + lambda I - sum_p W_ip Dinv_p W_jp^T; lanes over keyframe i's edges.  A point enters once per keyframe (at
// its first active edge there): two edges of one point at one keyframe add into one W block.  The diagonal wave also b_s = b_p - sum_p W_ip Dinv_p b_l.
__global__ void __launch_bounds__(64) k_lba_schur(LbaDev d) {
	int i = 0, q = blockIdx.x;
	while (q >= d.nFree - i) { q -= d.nFree - i; ++i; }
	const int j = i + q, lane = threadIdx.x;
	const int kfi = d.freeKf[i], kfj = d.freeKf[j], n = d.kfCount[i];
	const int* list = d.kfList + d.kfOff[i];
	double acc[42];
#pragma unroll
	for (int k = 0; k < 42; ++k) acc[k] = 0.0;
	for (int t = lane; t < n; t += 64) {
		const int e = list[t];
		if (!d.act[e]) continue;
		const int p = d.ept[e];
		int a, b;
		point_range(d, p, a, b);
		bool firstHere = true;
		for (int k = a; k < e && k < b; ++k) if (d.edgeKf[k] == kfi && d.act[k]) { firstHere = false; break; }
		if (!firstHere) continue;
		double Wi[6][3] = {}, Wj[6][3] = {};
		bool has = i == j;
		for (int k = a; k < b; ++k) {
			if (!d.act[k]) continue;
			const int kf = d.edgeKf[k];
			if (kf == kfi) add_w(d.edge + (size_t)k * kEdgeDoubles, Wi);
			else if (kf == kfj) { add_w(d.edge + (size_t)k * kEdgeDoubles, Wj); has = true; }
		}
		if (!has) continue;
		const double* Di = d.Dinv + 9 * (size_t)p;
		double T[6][3];
#pragma unroll
		for (int r = 0; r < 6; ++r)
#pragma unroll
			for (int c = 0; c < 3; ++c) T[r][c] = (Wi[r][0] * Di[c] + Wi[r][1] * Di[3 + c]) + Wi[r][2] * Di[6 + c];
#pragma unroll
		for (int r = 0; r < 6; ++r)
#pragma unroll
			for (int c = 0; c < 6; ++c) {
				const double* wj = i == j ? Wi[c] : Wj[c];
				acc[6 * r + c] += (T[r][0] * wj[0] + T[r][1] * wj[1]) + T[r][2] * wj[2];
			}
		if (i == j) {
			const double* db = d.db + 3 * (size_t)p;
#pragma unroll
			for (int r = 0; r < 6; ++r) acc[36 + r] += (Wi[r][0] * db[0] + Wi[r][1] * db[1]) + Wi[r][2] * db[2];
		}
	}
	wave_sum<42>(acc);
	if (lane != 0) return;
	const int N = 6 * d.nFree;
	const double lam = d.ctl->lm.lambda;
	for (int r = 0; r < 6; ++r)
		for (int c = 0; c < 6; ++c) {
			double h = 0.0;
			if (i == j) {
				const int lo = r < c ? r : c, hi = r < c ? c : r;
				h = d.Hpp[21 * i + (lo * 6 - lo * (lo - 1) / 2) + (hi - lo)] + (r == c ? lam : 0.0);
			}
			const double v = h - acc[6 * r + c];
			if (i == j) { if (c <= r) d.S[(size_t)(6 * i + r) * N + 6 * i + c] = v; }   // the solver reads the lower triangle
			else d.S[(size_t)(6 * j + c) * N + 6 * i + r] = v;
		}
	if (i == j) for (int r = 0; r < 6; ++r) d.bs[6 * i + r] = d.bp[6 * i + r] - acc[36 + r];
}

// one workgroup: unpivoted LDL^T of S (lower triangle, in place), the solve into xp.  Fails at the first pivot that is zero or not finite: xp is left alone.
__global__ void __launch_bounds__(1024) k_lba_solve(LbaDev d) {
	__shared__ double col[6 * kLbaMaxFree], y[6 * kLbaMaxFree], dd[6 * kLbaMaxFree];
	const int N = 6 * d.nFree, tid = threadIdx.x;
	double* S = d.S;
	bool ok = true;
	for (int j = 0; j < N; ++j) {
		const double dj = S[(size_t)j * N + j];
		if (dj == 0.0 || !finite_(dj)) { ok = false; break; }   // uniform
		if (tid == 0) dd[j] = dj;
		for (int r = j + 1 + tid; r < N; r += 1024) { const double l = S[(size_t)r * N + j] / dj; col[r] = l; S[(size_t)r * N + j] = l; }
		__syncthreads();
		const int m = N - j - 1;
		for (int t = tid; t < m * m; t += 1024) {
			const int rr = t / m, kk = t - rr * m;
			if (kk <= rr) S[(size_t)(j + 1 + rr) * N + j + 1 + kk] -= (col[j + 1 + rr] * col[j + 1 + kk]) * dj;
		}
		__syncthreads();
	}
	if (tid == 0) d.ctl->solveOk = ok ? 1 : 0;
	if (!ok) return;
	for (int r = tid; r < N; r += 1024) y[r] = d.bs[r];
	__syncthreads();
	for (int k = 0; k < N; ++k) {
		const double yk = y[k];
		__syncthreads();
		for (int r = k + 1 + tid; r < N; r += 1024) y[r] -= S[(size_t)r * N + k] * yk;
		__syncthreads();
	}
	for (int r = tid; r < N; r += 1024) y[r] = y[r] / dd[r];
	__syncthreads();
	for (int k = N - 1; k >= 0; --k) {
		const double yk = y[k];
		__syncthreads();
		for (int r = tid; r < k; r += 1024) y[r] -= S[(size_t)k * N + r] * yk;
		__syncthreads();
	}
	for (int r = tid; r < N; r += 1024) d.xp[r] = y[r];
}

// x_l = Dinv (b_l - W^T x_p) per active point (after a failed solve: the stale x), the trial estimates = estimates + x (oplus), the point's share of computeScale
__global__ void k_lba_apply(LbaDev d) {
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t < 6 * d.nKfs) {
		const int f = d.fidx[t / 6];
		d.poseT[t] = f >= 0 ? d.pose[t] + d.xp[6 * f + t % 6] : d.pose[t];
	}
	if (t >= d.nPoints) return;
	const int p = t;
	double* xl = d.xl + 3 * (size_t)p;
	if (!d.ptAct[p]) {
		for (int k = 0; k < 3; ++k) d.posT[3 * (size_t)p + k] = d.pos[3 * (size_t)p + k];
		return;
	}
	const double* bl = d.bl + 3 * (size_t)p;
	if (d.ctl->solveOk) {
		int a, b;
		point_range(d, p, a, b);
		double cl[3] = {bl[0], bl[1], bl[2]};
		for (int e = a; e < b; ++e) {
			if (!d.act[e]) continue;
			const int f = d.fidx[d.edgeKf[e]];
			if (f < 0) continue;
			const double* o = d.edge + (size_t)e * kEdgeDoubles;
			const double* x = d.xp + 6 * f;
			double s0 = 0.0, s1 = 0.0;
			for (int k = 0; k < 6; ++k) { s0 += o[k] * x[k]; s1 += o[6 + k] * x[k]; }
			for (int k = 0; k < 3; ++k) cl[k] -= o[20] * (o[12 + k] * s0 + o[15 + k] * s1);
		}
		const double* Di = d.Dinv + 9 * (size_t)p;
		for (int r = 0; r < 3; ++r) xl[r] = (Di[3 * r] * cl[0] + Di[3 * r + 1] * cl[1]) + Di[3 * r + 2] * cl[2];
	}
	const double lam = d.ctl->lm.lambda;
	double sc = 0.0;
	for (int k = 0; k < 3; ++k) {
		d.posT[3 * (size_t)p + k] = d.pos[3 * (size_t)p + k] + xl[k];
		sc += xl[k] * (lam * xl[k] + bl[k]);
	}
	d.ptScale[p] = sc;
}

// OptimizationAlgorithmLevenberg::solve behind the trial's evaluation, and — when the trial loop ends — its return value and the terminate action
__global__ void k_lba_decide(LbaDev d, int stopSeen, int it) {
	if (blockIdx.x || threadIdx.x) return;
	LbaCtl& c = *d.ctl;
	LmState& lm = c.lm;
	const double raw = c.sumChi;
	double scale = 0.0;
	for (int k = 0; k < 6 * d.nFree; ++k) scale += d.xp[k] * (lm.lambda * d.xp[k] + d.bp[k]);   // computeScale: all of x and b, poses then points
	scale += c.sumScale;                                                                       // the points' share, of k_lba_reduce
	c.accepted = lm_trial(lm, raw, c.solveOk != 0, scale) ? 1 : 0;
	if (c.accepted) lm.postChi = raw;   // an accepted trial's evaluation is the one the action will judge
	LbaRecord r{};
	r.more = lm_more(lm) && !stopSeen;
	r.resultOk = 1; r.why = STOP_ITERATIONS;
	if (!r.more) {
		if (const int end = lm_iter_end(lm)) { r.resultOk = 0; r.why = end; }
		// postIteration(it): the terminate action, on the errors of the current estimate
		if (lm_gain_stop(lm, it)) r.gainStop = 1;
	}
	r.qmax = lm.qmax; r.nonfinite = c.nonfinite; r.nActive = c.nActive; r.accepted = c.accepted;
	r.lambda = lm.lambda; r.chi2 = lm.lastChi; r.nErased[0] = c.nErased[0]; r.nErased[1] = c.nErased[1];   // chi2: what the action last judged
	*d.rec = r;
}

__global__ void k_lba_accept(LbaDev d) {
	if (!d.ctl->accepted) return;
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t < 6 * d.nKfs) d.pose[t] = d.poseT[t];
	if (t < 3 * d.nPoints) d.pos[t] = d.posT[t];
}

// ---------------------------------------------------------------------------------------------- the passes and the outputs
// :764-783 / :795-816 on the plain chi2 of the latest evaluation: sequential inside a point
__global__ void k_lba_outlier(LbaDev d, int rnd) {
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= d.nPoints) return;
	int a, b;
	point_range(d, p, a, b);
	bool bad = d.ptBad[p] != 0;
	int total = d.ptTotal[p], erased = 0, left = 0;
	for (int e = a; e < b; ++e) {
		if (d.level[e] != 0) continue;
		if (!bad && d.eChi[e] > d.dsqr) {   // thHuber^2 is the same product as the kernel's delta^2
			d.level[e] = 1;
			d.state[e] = (uint8_t)(rnd + 1);
			++erased;
			if (--total < 2) bad = true;   // EraseObservation: nrObs < 2 -> SetBadFlag
		} else ++left;
	}
	d.ptBad[p] = bad;
	d.ptTotal[p] = total;
	if (erased) atomicAdd(&d.ctl->nErased[rnd], erased);
	if (left) atomicAdd(&d.ctl->nActive, left);
}

__global__ void k_lba_record(LbaDev d) {
	if (blockIdx.x || threadIdx.x) return;
	const LbaCtl& c = *d.ctl;
	LbaRecord r{};
	r.nonfinite = c.nonfinite; r.nActive = c.nActive; r.lambda = c.lm.lambda; r.chi2 = c.lm.lastChi; r.nErased[0] = c.nErased[0]; r.nErased[1] = c.nErased[1];
	*d.rec = r;
}

// full: poses, kf_t, the positions of the points that are written back, both state arrays; else (round two failed) the states alone
__global__ void k_lba_writeback(LbaDev d, int full) {
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t < d.nEdges) d.edgeStateOut[t] = d.state[t];
	if (full && t < 6 * d.nLocal) d.kfPoseIO[t] = d.pose[t];
	if (full && d.kfT && t < 3 * d.nLocal) d.kfT[t] = d.pose[6 * (t / 3) + 3 + t % 3];   // Hom2T of cayley2hom(pose)
	if (t >= d.nPoints) return;
	uint8_t st = PT_KEPT;
	if (d.ptBad[t]) st = PT_BAD;
	else if (full && d.ptTotal[t] - (d.badObs ? d.badObs[t] : 0) > 1 && d.ptDeg[t] >= 2) {
		st = PT_WRITTEN;
		for (int k = 0; k < 3; ++k) d.posIO[3 * (size_t)t + k] = d.pos[3 * (size_t)t + k];
	}
	d.ptStateOut[t] = st;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- cOptimizer::LocalBundleAdjustment
int mcs_local_bundle_adjustment(mcs_ctx* c, int n_kfs, int n_local, double* kf_pose_min, const uint8_t* kf_fixed, double* kf_t, int n_points, double* pos,
                                const int32_t* pt_first, int n_edges, const int32_t* edge_kf, const int32_t* edge_cam, const mcs_keypoint* edge_key,
                                const int32_t* pt_total_obs, const int32_t* pt_bad_obs, const double* M_c_min, const mcs_ocam* cams, int nr_cams,
                                const double* inv_level_sigma2, int nlevels, double std_recon, int* stop_flag, mcs_mem_kind kind, uint8_t* edge_state,
                                uint8_t* pt_state, mcs_lba_diag* diag) {
	const LbaCall q{n_kfs, n_local, kf_pose_min, kf_fixed, kf_t, n_points, pos, pt_first, n_edges, edge_kf, edge_cam, edge_key, pt_total_obs, pt_bad_obs,
	                M_c_min, cams, nr_cams, inv_level_sigma2, nlevels, std_recon, stop_flag, kind, edge_state, pt_state, diag};
	if (int r = guard_lba(c, q, c && c->asyncSearch)) return r;
	const bool host = kind == MCS_MEM_HOST;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	// who is free: the one thing the host must know before anything runs (the capacity of the reduced system)
	std::vector<uint8_t> fixedH((size_t)n_kfs);
	if (n_kfs) {
		if (host) memcpy(fixedH.data(), kf_fixed, (size_t)n_kfs);
		else {
			if (int r = ctx_join_greedy(c, s)) return r;
			HIPCHK(hipMemcpyAsync(fixedH.data(), kf_fixed, (size_t)n_kfs, hipMemcpyDeviceToHost, s));
			HIPCHK(hipStreamSynchronize(s));
		}
	}
	int nFree = 0;
	if (int r = guard_lba_free(fixedH.data(), n_kfs, &nFree)) return r;
	if (host)
		if (int r = guard_lba_content(q)) return r;
	mcs_lba_diag dg{};
	dg.stop[0] = dg.stop[1] = STOP_NOT_RUN;
	dg.n_free = nFree;
	auto leave = [&](int status) { dg.status = status; if (diag) *diag = dg; return MCS_OK; };
	if (n_local < 2) return leave(MCS_LBA_TOO_FEW);                 // :489
	bool aux = false;                                               // the action's own flag (pbStopFlag == NULL)
	auto stopped = [&]() { return stop_flag ? *stop_flag != 0 : aux; };
	if (stop_flag && *stop_flag) return leave(MCS_LBA_STOPPED);     // :739-741
	if (nFree == 0) return leave(MCS_LBA_NO_FREE_POSE);
	if (!c->lbaRec) HIPCHK(hipHostMalloc(&c->lbaRec, sizeof(LbaRecord), hipHostMallocDefault));
	volatile LbaRecord* rec = (volatile LbaRecord*)c->lbaRec;

	std::vector<int> fidx((size_t)n_kfs, -1), freeKf;
	for (int k = 0; k < n_kfs; ++k) if (!fixedH[k]) { fidx[k] = (int)freeKf.size(); freeKf.push_back(k); }
	const size_t K = n_kfs, P = n_points, E = n_edges, F = nFree, nr = nr_cams, N = 6 * F;
	LbaDev d{};
	d.nKfs = n_kfs; d.nLocal = n_local; d.nPoints = n_points; d.nEdges = n_edges; d.nrCams = nr_cams; d.nlevels = nlevels; d.nFree = nFree;
	d.delta = 1.345 * std_recon; d.dsqr = d.delta * d.delta;
	d.rec = (LbaRecord*)device_view(c->lbaRec);
	if (!d.rec) return fail(MCS_ERR_HIP, "the control record is not visible from the device");
	Staging st(c, host);
	st.inout(&d.kfPoseIO, kf_pose_min, K * 48);   // kf_fixed reaches the device as fidx / freeKf
	if (kf_t) st.inout(&d.kfT, kf_t, (size_t)n_local * 24);
	st.inout(&d.posIO, pos, P * 24); st.in(&d.ptFirst, pt_first, (P + 1) * 4);
	st.in(&d.edgeKf, edge_kf, E * 4); st.in(&d.edgeCam, edge_cam, E * 4); st.in(&d.key, edge_key, E * sizeof(mcs_keypoint));
	st.in(&d.totalObs, pt_total_obs, P * 4); st.in(&d.badObs, pt_bad_obs, P * 4);
	st.in(&d.McMin, M_c_min, nr * 48); st.in(&d.cams, cams, nr * sizeof(mcs_ocam)); st.in(&d.invSigma2, inv_level_sigma2, (size_t)nlevels * 8);
	st.inout(&d.edgeStateOut, edge_state, E); st.inout(&d.ptStateOut, pt_state, P);   // in/out: a status that writes nothing leaves them as they came in
	st.upload(&d.fidx, fidx.data(), K * 4); st.upload(&d.freeKf, freeKf.data(), F * 4);
	st.scratch(&d.cam, nr * sizeof(OcamDev)); st.scratch(&d.dInvP, nr * MCS_MAX_POLY * 8); st.scratch(&d.McH, nr * 128);
	st.scratch(&d.pose, K * 48); st.scratch(&d.poseT, K * 48); st.scratch(&d.pos, P * 24); st.scratch(&d.posT, P * 24);
	st.scratch(&d.rig, K * nr * kRigDoubles * 8);
	st.scratch(&d.ept, E * 4); st.scratch(&d.level, E); st.scratch(&d.act, E); st.scratch(&d.state, E);
	st.scratch(&d.edge, E * kEdgeDoubles * 8); st.scratch(&d.eChi, E * 8);
	st.scratch(&d.Hll, P * 48); st.scratch(&d.bl, P * 24); st.scratch(&d.ptChi, P * 8); st.scratch(&d.Dinv, P * 72); st.scratch(&d.db, P * 24);
	st.scratch(&d.xl, P * 24); st.scratch(&d.ptScale, P * 8);
	st.scratch(&d.ptAct, P * 4); st.scratch(&d.ptDeg, P * 4); st.scratch(&d.ptTotal, P * 4); st.scratch(&d.ptBad, P);
	st.scratch(&d.Hpp, F * 21 * 8); st.scratch(&d.bp, F * 48); st.scratch(&d.xp, N * 8);
	st.scratch(&d.kfCount, F * 4); st.scratch(&d.kfOff, (F + 1) * 4); st.scratch(&d.kfList, E * 4);
	st.scratch(&d.S, N * N * 8); st.scratch(&d.bs, N * 8);
	st.scratch(&d.ctl, sizeof(LbaCtl));
	if (int r = st.commit()) return r;

	int status = MCS_LBA_OK;
	auto sync = [&]() -> int { HIPCHK(hipStreamSynchronize(s)); return MCS_OK; };
	auto run = [&]() -> int {
		c->tic("local_bundle_adjustment");
		HIPCHK(hipMemsetAsync(d.ctl, 0, sizeof(LbaCtl), s));
		HIPCHK(hipMemsetAsync(d.level, 1, E ? E : 1, s)); HIPCHK(hipMemsetAsync(d.ept, 0xff, E ? E * 4 : 1, s));
		HIPCHK(hipMemsetAsync(d.act, 0, E ? E : 1, s)); HIPCHK(hipMemsetAsync(d.state, 0, E ? E : 1, s));
		HIPCHK(hipMemcpyAsync(d.pose, d.kfPoseIO, K * 48, hipMemcpyDeviceToDevice, s));
		if (P) HIPCHK(hipMemcpyAsync(d.pos, d.posIO, P * 24, hipMemcpyDeviceToDevice, s));
		hipLaunchKernelGGL(k_lba_cams, blocks(nr, 64), dim3(64), 0, s, d);
		hipLaunchKernelGGL(k_lba_prepare, blocks(P, 256), dim3(256), 0, s, d);
		hipLaunchKernelGGL(k_lba_kf_lists<false>, dim3(nFree), dim3(256), 0, s, d);
		hipLaunchKernelGGL(k_lba_kf_offsets, dim3(1), dim3(64), 0, s, d);
		hipLaunchKernelGGL(k_lba_kf_lists<true>, dim3(nFree), dim3(256), 0, s, d);
		hipLaunchKernelGGL(k_lba_record, dim3(1), dim3(64), 0, s, d);
		if (int r = sync()) return r;
		int nActive = rec->nActive;
		dg.n_edges1 = nActive;
		const size_t big = std::max(std::max(6 * K, 3 * P), E);
		bool firstEval = true;
		auto evaluate = [&](const double* poses, const double* pts, bool build) {
			hipLaunchKernelGGL(k_lba_rigs, blocks(K * nr, 128), dim3(128), 0, s, d, poses, build ? 1 : 0, firstEval ? 0 : 1);
			firstEval = false;
			if (build) hipLaunchKernelGGL(k_lba_linearise<true>, blocks(P, 4), dim3(256), 0, s, d, poses, pts);
			else hipLaunchKernelGGL(k_lba_linearise<false>, blocks(P, 4), dim3(256), 0, s, d, poses, pts);
		};
		for (int rnd = 0; rnd < 2; ++rnd) {
			if (nActive == 0) {   // optimize() returns Fail (:750-754, :788-792): no write-back; the erasures of pass one are the caller's already
				status = MCS_LBA_FAILED;
				if (rnd == 1) hipLaunchKernelGGL(k_lba_writeback, blocks(big, 256), dim3(256), 0, s, d, 0);
				return MCS_OK;
			}
			HIPCHK(hipMemsetAsync(d.xp, 0, N * 8, s));                   // buildStructure -> Solver::resize: zeros
			if (P) HIPCHK(hipMemsetAsync(d.xl, 0, P * 24, s));
			const int maxIt = rnd == 0 ? 10 : 15;
			int it = 0, why = stopped() ? STOP_NOT_RUN : STOP_ITERATIONS;
			bool resultOk = true;
			while (it < maxIt && !stopped() && resultOk) {
				// ---- OptimizationAlgorithmLevenberg::solve(it): computeActiveErrors, buildSystem
				const bool first = rnd == 0 && it == 0;
				evaluate(d.pose, d.pos, true);
				hipLaunchKernelGGL(k_lba_reduce, dim3(1), dim3(1024), 0, s, d, 1);
				hipLaunchKernelGGL(k_lba_pose_blocks, dim3(nFree), dim3(256), 0, s, d);
				hipLaunchKernelGGL(k_lba_iter_begin, dim3(1), dim3(64), 0, s, d, first ? 1 : 0, it);
				while (true) {
					const int stopSeen = stopped() ? 1 : 0;   // the caller's flag as this trial reads it
					hipLaunchKernelGGL(k_lba_dinv, blocks(P, 256), dim3(256), 0, s, d);
					hipLaunchKernelGGL(k_lba_schur, dim3(nFree * (nFree + 1) / 2), dim3(64), 0, s, d);
					hipLaunchKernelGGL(k_lba_solve, dim3(1), dim3(1024), 0, s, d);
					hipLaunchKernelGGL(k_lba_apply, blocks(big, 256), dim3(256), 0, s, d);
					evaluate(d.poseT, d.posT, false);
					hipLaunchKernelGGL(k_lba_reduce, dim3(1), dim3(1024), 0, s, d, 0);
					hipLaunchKernelGGL(k_lba_decide, dim3(1), dim3(64), 0, s, d, stopSeen, it);
					hipLaunchKernelGGL(k_lba_accept, blocks(big, 256), dim3(256), 0, s, d);
					if (int r = sync()) return r;   // the one wait of the trial
					if (first && rec->nonfinite) { status = MCS_LBA_NONFINITE; return MCS_OK; }
					if (!rec->more) break;
				}
				dg.trials[rnd][it] = rec->qmax;
				if (!rec->resultOk) { resultOk = false; why = rec->why; }
				if (rec->gainStop) {   // setOptimizerStopFlag(true): through the caller's pointer where there is one
					if (stop_flag) *stop_flag = 1; else aux = true;
					if (resultOk) why = STOP_GAIN;
				}
				dg.lambda = rec->lambda; dg.chi2 = rec->chi2;
				++it;
			}
			dg.iters[rnd] = it; dg.stop[rnd] = why;
			if (rnd == 0 && stop_flag && *stop_flag) { status = MCS_LBA_STOPPED; return MCS_OK; }   // :756-762: nothing at all is written back
			// ---- the pass behind this round, on the errors of the current estimate
			evaluate(d.pose, d.pos, false);
			HIPCHK(hipMemsetAsync(&d.ctl->nActive, 0, sizeof(int), s));
			hipLaunchKernelGGL(k_lba_outlier, blocks(P, 256), dim3(256), 0, s, d, rnd);
			hipLaunchKernelGGL(k_lba_record, dim3(1), dim3(64), 0, s, d);
			if (int r = sync()) return r;
			nActive = rec->nActive;
			dg.n_erased[0] = rec->nErased[0]; dg.n_erased[1] = rec->nErased[1];
		}
		hipLaunchKernelGGL(k_lba_writeback, blocks(big, 256), dim3(256), 0, s, d, 1);
		return MCS_OK;
	};
	int rc = run();
	c->toc("local_bundle_adjustment");
	if (rc == MCS_OK && hipGetLastError() != hipSuccess) rc = fail(MCS_ERR_HIP, "local bundle adjustment: a launch failed");
	c->lastResultStream = s;
	rc = st.finish(rc);   // a status that writes nothing leaves the in/out pieces as they were uploaded
	if (rc != MCS_OK) return rc;
	return leave(status);
}
