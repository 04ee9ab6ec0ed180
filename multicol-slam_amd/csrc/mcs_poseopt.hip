// mcs_poseopt.hip — cOptimizer::PoseOptimization (src/cOptimizer.cpp:259-459) for a batch of independent problems: one workgroup per problem, both rounds of the
// reference's g2o run in one launch, and the entry point mcs_pose_optimization (include/mcs_c.h).  DESIGN.md 4l; the statement-by-statement restatement the
// kernel is held to is tests/poseopt_model.py.  The Levenberg-Marquardt steps, the Huber pair, the 6x6 solve and the ordered sums are csrc/mcs_lm.h's, the
// matrices, the camera and the derivatives csrc/mcs_geom.h's.
//
// The edges (features with a map point) are strided over the threads: thread t owns features t, t + kPoseThreads, ... in every pass, and sums them in ascending
// order.  A pass reduces within a wave by shuffles, then across the waves through LDS in wave order, so a problem's sums do not depend on the batch or the run.
// Lane 0 keeps the Levenberg-Marquardt state, factorises the 6x6 and broadcasts the step and every decision through LDS; control flow is uniform.
//
// No edge keeps its error between passes: the terminate action recomputes the active errors before it reads them (sparse_optimizer_terminate_action.cpp:29),
// after every iteration, so whatever reads an edge's error — the gain test, both outlier passes — reads the error of the CURRENT estimate, and a pass at that
// estimate gives it again.  The one per-edge state is its level, which is the outlier flag of the first pass.
//
// The Jacobian is derived here by the chain rule (the reference's is generated code and is not used in any form): with Mct = Mt * Mc the camera-frame point is
// p = Rc^T Rt^T (X - t) - Rc^T tc, so dp/dt = -(Rt Rc)^T and dp/dc_i = Rc^T (dRt/dc_i)^T (X - t); d(u, v)/dp differentiates WorldToImg; e = z - (u, v).
#include "mcs_poseopt.h"
#include "mcs_geom.h"
#include "mcs_lm.h"

using namespace mcs;

namespace {

constexpr int kWaves = kPoseThreads / 64;
constexpr int kSums = 28;   // 21 of H (upper triangle, row-major), 6 of b, 1 of the robust chi2

struct PoseShared {
	OcamDev cam[32];
	double dInvP[32][MCS_MAX_POLY];   // coefficients of d rho / d theta
	double McH[32][16];               // cayley2hom(M_c_min[c])
	double inv[32][16];               // invMat(Mt * Mc[c]) at the current estimate
	double A[32][3][9];               // Rc^T (dRt/dc_i)^T, build passes only
	double red[kWaves][kSums];
	double tot[kSums];
	double H[21], b[6];               // of the iteration's build pass (lane 0 reads them in every trial)
	double pose[6], backup[6], x[6];
	int nInit, nonfinite, nBad, go, cont;
};

// Mct and its inverse of camera c at `pose` (EdgeProjectXYZ2MCS::computeError, Set_M_t_from_min); Build: also A_i = Rc^T (dRt/dc_i)^T
template <bool Build>
__device__ void camera_state(PoseShared& sh, int c, const double* pose, double* MtMcOut) {
	double Mt[16], Mct[16];
	cayley2hom(pose, Mt);
	matx44_mul(Mt, sh.McH[c], Mct);
	inv_mat(Mct, sh.inv[c]);
	if (MtMcOut) for (int k = 0; k < 16; ++k) MtMcOut[k] = Mct[k];
	if (Build) cayley_rot_factors(pose, Mt, sh.McH[c], &sh.A[c][0][0]);
}

__device__ __forceinline__ bool edge_of(const PoseArgs& a, const mcs_keypoint* keys, const int* cam, const int* points, int i, int& pid, int& c, int& oct) {
	pid = points[i];
	if (pid < 0 || pid >= a.npoints) return false;
	c = cam[i]; oct = keys[i].octave;
	return c >= 0 && c < a.nrCams && oct >= 0 && oct < a.nlevels;
}

struct Edges { const mcs_keypoint* keys; const int* cam; const int* points; uint8_t* outlier; int n; };

// One pass over the active edges at the estimate behind sh.inv (and sh.A): the robust chi2 (activeRobustChi2), Build: also H and b (constructQuadraticForm).
// levelZero: only edges whose outlier flag is clear (initializeOptimization(0)).
template <bool Build>
__device__ void pass(PoseShared& sh, const PoseArgs& a, const Edges& e, bool levelZero, double delta, double dsqr) {
	double acc[Build ? kSums : 1];
#pragma unroll
	for (int k = 0; k < (Build ? kSums : 1); ++k) acc[k] = 0.0;
	bool bad = false;
	for (int i = threadIdx.x; i < e.n; i += kPoseThreads) {
		int pid, c, oct;
		if (!edge_of(a, e.keys, e.cam, e.points, i, pid, c, oct)) continue;
		if (levelZero && e.outlier[i]) continue;
		const double X[3] = {a.pos[3 * (size_t)pid], a.pos[3 * (size_t)pid + 1], a.pos[3 * (size_t)pid + 2]};
		double p[3], u, v;
		matx44_point<3>(sh.inv[c], X, p);   // the camera-frame point of the edge
		omni_world_to_img(sh.cam[c], p[0], p[1], p[2], u, v);
		const double e0 = (double)e.keys[i].x - u, e1 = (double)e.keys[i].y - v;
		const double w = a.invSigma2[oct];
		const double c2 = e0 * (w * e0) + e1 * (w * e1);   // _error.dot(information() * _error)
		double rho0, rho1;
		huber_robustify(c2, delta, dsqr, rho0, rho1);
		if constexpr (!Build) { (void)rho1; acc[0] += rho0; }
		else {
		double D[2][3], J[2][6];
		d_world_to_img(sh.cam[c], sh.dInvP[c], p[0], p[1], p[2], D);
		const double d[3] = {X[0] - sh.pose[3], X[1] - sh.pose[4], X[2] - sh.pose[5]};
#pragma unroll
		for (int k = 0; k < 6; ++k) {
			double dp[3];
#pragma unroll
			for (int r = 0; r < 3; ++r)
				dp[r] = k < 3 ? sh.A[c][k][3 * r] * d[0] + sh.A[c][k][3 * r + 1] * d[1] + sh.A[c][k][3 * r + 2] * d[2] : -sh.inv[c][4 * r + (k - 3)];
			J[0][k] = -(D[0][0] * dp[0] + D[0][1] * dp[1] + D[0][2] * dp[2]);
			J[1][k] = -(D[1][0] * dp[0] + D[1][1] * dp[1] + D[1][2] * dp[2]);
			bad |= !finite_(J[0][k]) || !finite_(J[1][k]);
		}
		bad |= !finite_(e0) || !finite_(e1) || !finite_(w);
		const double rw = rho1 * w;   // robustInformation = rho[1] * information; no second-order term
		int s = 0;
#pragma unroll
		for (int r = 0; r < 6; ++r)
#pragma unroll
			for (int q = r; q < 6; ++q) acc[s++] += rw * (J[0][r] * J[0][q] + J[1][r] * J[1][q]);
#pragma unroll
		for (int r = 0; r < 6; ++r) acc[21 + r] += -rw * (J[0][r] * e0 + J[1][r] * e1);
		acc[27] += rho0;
		}
	}
	if (Build && bad) atomicOr(&sh.nonfinite, 1);
	block_sums<Build ? kSums : 1>(acc, sh.red, sh.tot);
}

// :412-427 / :433-447: chi2 > thHuber2 of every edge still at level 0, at the estimate behind sh.inv
__device__ void outlier_pass(PoseShared& sh, const PoseArgs& a, const Edges& e, double th2) {
	int nbad = 0;
	for (int i = threadIdx.x; i < e.n; i += kPoseThreads) {
		int pid, c, oct;
		if (!edge_of(a, e.keys, e.cam, e.points, i, pid, c, oct) || e.outlier[i]) continue;
		const double X[3] = {a.pos[3 * (size_t)pid], a.pos[3 * (size_t)pid + 1], a.pos[3 * (size_t)pid + 2]};
		double p[3], u, v;
		matx44_point<3>(sh.inv[c], X, p);   // the camera-frame point of the edge
		omni_world_to_img(sh.cam[c], p[0], p[1], p[2], u, v);
		const double e0 = (double)e.keys[i].x - u, e1 = (double)e.keys[i].y - v;
		const double w = a.invSigma2[oct];
		if (e0 * (w * e0) + e1 * (w * e1) > th2) { e.outlier[i] = 1; ++nbad; }
	}
	if (nbad) atomicAdd(&sh.nBad, nbad);
	__syncthreads();
}

__global__ void __launch_bounds__(kPoseThreads) k_poseopt(PoseArgs a, PoseChunk ch, int first) {
	__shared__ PoseShared sh;
	const int tid = threadIdx.x, lp = blockIdx.x, gp = first + lp, nr = a.nrCams;
	const Edges e{ch.keys[lp], ch.cam[lp], ch.points[lp], ch.outlier[lp], ch.n[lp]};
	double* const poseOut = a.poseMin + 6 * (size_t)gp;

	if (tid < nr) {
		const mcs_ocam& m = a.cams[tid];
		const OcamDev o = ocam_dev_of(m);
		sh.cam[tid] = o;
		ocam_dinvp(m, o, sh.dInvP[tid]);
		cayley2hom(a.McMin + 6 * tid, sh.McH[tid]);
	}
	if (tid == 0) {
		for (int k = 0; k < 6; ++k) { sh.pose[k] = poseOut[k]; sh.x[k] = 0.0; }
		sh.nInit = 0; sh.nonfinite = 0; sh.nBad = 0;
	}
	int mine = 0;
	for (int i = tid; i < e.n; i += kPoseThreads) {
		int pid, c, oct;
		e.outlier[i] = 0;   // :351
		mine += edge_of(a, e.keys, e.cam, e.points, i, pid, c, oct) ? 1 : 0;
	}
	__syncthreads();
	if (mine) atomicAdd(&sh.nInit, mine);
	__syncthreads();
	const int nInit = sh.nInit;

	const double delta = 1.345 * a.huber[gp], dsqr = delta * delta, th2 = delta * delta;
	// lane 0's state
	int status = MCS_POSE_OK, iters[2] = {0, 0}, stop[2] = {STOP_NOT_RUN, STOP_NOT_RUN}, trials[2][10] = {};
	LmState lm{};
	lm.lambda = -1.0; lm.ni = 2.0;
	bool stopFlag = false;

	if (nInit > 0) {   // uniform
		for (int rnd = 0; rnd < 2; ++rnd) {
			const int nAct = nInit - sh.nBad;   // round 1: the edges the first outlier pass left at level 0
			bool resultOk = true;
			int it = 0, why = stopFlag || nAct == 0 ? STOP_NOT_RUN : STOP_ITERATIONS;
			if (tid == 0) for (int k = 0; k < 6; ++k) sh.x[k] = 0.0;   // Solver::resize: zeros
			while (true) {
				if (tid == 0) sh.go = it < 10 && !stopFlag && resultOk && nAct > 0;
				__syncthreads();
				if (!sh.go) break;
				// ---- OptimizationAlgorithmLevenberg::solve(it)
				if (tid < nr) camera_state<true>(sh, tid, sh.pose, nullptr);
				__syncthreads();
				pass<true>(sh, a, e, rnd == 1, delta, dsqr);
				if (rnd == 0 && it == 0) {   // the screen of the first evaluation: every edge's residual, Jacobian and weight, the Huber pair, the sums
					bool nf = sh.nonfinite || !finite_(delta) || !finite_(dsqr);
					for (int k = 0; k < kSums; ++k) nf |= !finite_(sh.tot[k]);
					if (nf) { status = MCS_POSE_NONFINITE; break; }   // uniform: not optimised
				}
				lm_iter_begin(lm, sh.tot[27]);   // every thread: written by lane 0 alone, the iteration's values would stay live around the loop in the others
				lm.rho = 0.0;                    // solve()'s "double rho=0;", for the same reason: lm_trial writes it before anything reads it
				if (tid == 0) {
					for (int k = 0; k < 21; ++k) sh.H[k] = sh.tot[k];
					for (int k = 0; k < 6; ++k) sh.b[k] = sh.tot[21 + k];
					if (it == 0) lm_start(lm, lm_lambda_init(max_abs_diag<6>(sh.H, 0.0)));
				}
				while (true) {
					bool ok2 = true;
					if (tid == 0) {
						double x[6];
						for (int k = 0; k < 6; ++k) { x[k] = sh.x[k]; sh.backup[k] = sh.pose[k]; }   // push
						ok2 = ldlt_solve<6>(sh.H, lm.lambda, sh.b, x);
						for (int k = 0; k < 6; ++k) { sh.x[k] = x[k]; sh.pose[k] = sh.pose[k] + x[k]; }   // oplus, with the stale x after a failed solve
					}
					__syncthreads();
					if (tid < nr) camera_state<false>(sh, tid, sh.pose, nullptr);
					__syncthreads();
					pass<false>(sh, a, e, rnd == 1, delta, dsqr);
					if (tid == 0) {
						const double rawChi = sh.tot[0];
						double scale = 0.0;   // computeScale: the six of x and b
						for (int j = 0; j < 6; ++j) scale += sh.x[j] * (lm.lambda * sh.x[j] + sh.b[j]);
						if (lm_trial(lm, rawChi, ok2, scale)) lm.postChi = rawChi;   // an accepted trial's pass evaluated the estimate the action will judge
						else for (int k = 0; k < 6; ++k) sh.pose[k] = sh.backup[k];   // pop
						sh.cont = lm_more(lm) && !stopFlag;
					}
					__syncthreads();
					if (!sh.cont) break;
				}
				if (tid == 0) {
					trials[rnd][it] = lm.qmax;
					if (const int end = lm_iter_end(lm)) { resultOk = false; why = end; }
					// ---- postIteration(it): the terminate action, on the errors of the current estimate (postChi: the chi2 of the pass that evaluated it)
					if (lm_gain_stop(lm, it)) { stopFlag = true; if (resultOk) why = STOP_GAIN; }   // never cleared: this g2o has no iteration -1 call
				}
				++it;
			}
			if (status != MCS_POSE_OK) break;
			iters[rnd] = it; stop[rnd] = why;
			// ---- the outlier pass behind this round, at the current estimate
			__syncthreads();
			if (tid < nr) camera_state<false>(sh, tid, sh.pose, nullptr);
			__syncthreads();
			outlier_pass(sh, a, e, th2);
		}
	}
	__syncthreads();
	if (status == MCS_POSE_NONFINITE && tid == 0) for (int k = 0; k < 6; ++k) sh.pose[k] = poseOut[k];   // nothing was applied yet; for the matrices below
	__syncthreads();
	// Set_M_t_from_min (src/cam_system_omni.cpp:170-183)
	if (tid < nr) {
		double MtMc[16];
		camera_state<false>(sh, tid, sh.pose, MtMc);
		const size_t at = ((size_t)gp * nr + tid) * 16;
		if (a.MtMc) for (int k = 0; k < 16; ++k) a.MtMc[at + k] = MtMc[k];
		if (a.MtMcInv) for (int k = 0; k < 16; ++k) a.MtMcInv[at + k] = sh.inv[tid][k];
	}
	if (tid == 0) {
		const int nBad = status == MCS_POSE_OK ? sh.nBad : 0;
		for (int k = 0; k < 6; ++k) poseOut[k] = sh.pose[k];
		a.nInliers[gp] = nInit - nBad;
		a.share[gp] = nInit > 0 ? (double)nBad / (double)nInit : 0.0;   // the `inliers` out-parameter (:454-456)
		if (a.diag) {
			mcs_pose_diag& g = a.diag[gp];
			g.status = status; g.pad = 0;
			for (int r = 0; r < 2; ++r) { g.iters[r] = iters[r]; g.stop[r] = stop[r]; for (int k = 0; k < 10; ++k) g.trials[r][k] = trials[r][k]; }
			g.lambda = nInit > 0 && status == MCS_POSE_OK ? lm.lambda : 0.0; g.chi2 = status == MCS_POSE_OK ? lm.lastChi : 0.0;
		}
	}
}

}  // namespace

namespace mcs {
void launch_poseopt(const PoseArgs& a, const PoseChunk& ch, int first, int count, hipStream_t s) {
	hipLaunchKernelGGL(k_poseopt, dim3(count), dim3(kPoseThreads), 0, s, a, ch, first);
}
}  // namespace mcs

// ---------------------------------------------------------------------------------------------- cOptimizer::PoseOptimization
int mcs_pose_optimization(mcs_ctx* c, int nproblems, const mcs_pose_frame* frames, const mcs_point_table* pts, const double* M_c_min, const mcs_ocam* cams,
                          int nr_cams, const double* inv_level_sigma2, int nlevels, const double* huber_multiplier, mcs_mem_kind kind, double* pose_min,
                          double* MtMc, double* MtMc_inv, uint8_t* const* outlier, int32_t* n_inliers, double* outlier_share, mcs_pose_diag* diag) {
	const PoseCall q{nproblems, frames, pts, M_c_min, cams, nr_cams, inv_level_sigma2, nlevels, huber_multiplier, kind,
	                 pose_min, MtMc, MtMc_inv, outlier, n_inliers, outlier_share, diag};
	if (int r = guard_pose(c, q, c && c->asyncSearch)) return r;
	if (nproblems == 0) return MCS_OK;
	const bool host = kind == MCS_MEM_HOST;
	if (host)
		if (int r = guard_pose_content(q)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (int r = ctx_join_greedy(c, s)) return r;   // the points may come from a search whose greedy pass runs on the side stream
	const size_t np = nproblems, nr = nr_cams;
	PoseArgs a{};
	a.npoints = pts->n; a.nrCams = nr_cams; a.nlevels = nlevels;
	std::vector<const mcs_keypoint*> keys(np); std::vector<const int*> cam(np), points(np); std::vector<uint8_t*> out(np);
	Staging st(c, host);
	st.in(&a.pos, pts->pos, (size_t)pts->n * 24); st.in(&a.McMin, M_c_min, nr * 48); st.in(&a.cams, cams, nr * sizeof(mcs_ocam));
	st.in(&a.invSigma2, inv_level_sigma2, (size_t)nlevels * 8); st.in(&a.huber, huber_multiplier, np * 8);
	st.inout(&a.poseMin, pose_min, np * 48);
	if (MtMc) st.out(&a.MtMc, MtMc, np * nr * 128);
	if (MtMc_inv) st.out(&a.MtMcInv, MtMc_inv, np * nr * 128);
	st.out(&a.nInliers, n_inliers, np * 4); st.out(&a.share, outlier_share, np * 8);
	if (diag) st.out(&a.diag, diag, np * sizeof(mcs_pose_diag));
	for (size_t p = 0; p < np; ++p) {
		const size_t n = frames[p].n;
		st.in(&keys[p], frames[p].keys, n * sizeof(mcs_keypoint)); st.in(&cam[p], frames[p].cam, n * 4); st.in(&points[p], frames[p].points, n * 4);
		if (n) st.out(&out[p], outlier[p], n); else out[p] = nullptr;
	}
	if (int r = st.commit()) return r;
	c->tic("pose_optimization");
	for (int first = 0; first < nproblems; first += kPoseBatch) {
		const int count = std::min(kPoseBatch, nproblems - first);
		PoseChunk ch{};
		for (int k = 0; k < count; ++k) {
			ch.keys[k] = keys[first + k]; ch.cam[k] = cam[first + k]; ch.points[k] = points[first + k]; ch.outlier[k] = out[first + k]; ch.n[k] = frames[first + k].n;
		}
		launch_poseopt(a, ch, first, count, s);
	}
	c->toc("pose_optimization");
	c->lastResultStream = s;   // every output is complete on the context's stream
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}
