// mcs_sim3opt.hip — cOptimizer::OptimizeSim3 (src/cOptimizerLoopStuff.cpp:58-264) for a batch of independent loop candidates: one workgroup per problem, both
// rounds of the reference's g2o run in one launch, and the entry point mcs_sim3_optimize (include/mcs_c.h).  DESIGN.md 4m; the statement-by-statement
// restatement the kernel is held to is tests/sim3opt_model.py.  The Sim3 arithmetic is csrc/mcs_sim3g.h, the camera and the matrices csrc/mcs_geom.h, the
// Levenberg-Marquardt steps, the Huber pair, the 7x7 solve and the ordered sums csrc/mcs_lm.h.
//
// The correspondences are strided over the threads: thread t owns correspondences t, t + kSim3OptThreads, ... in every pass and adds them in ascending order,
// edge e12 before edge e21 (the order of the optimiser's active edges).  A pass reduces within a wave by shuffles, then across the waves through LDS in wave
// order, so a problem's sums do not depend on the batch or the run.  Lane 0 keeps the Levenberg-Marquardt state, factorises the 7x7 and broadcasts the
// estimate and every decision through LDS; control flow is uniform.
//
// The Jacobian is the reference's: g2o's central differences (core/base_binary_edge.hpp:130-205), column d = (e(Sim3(+1e-9 e_d) * S) - e(Sim3(-1e-9 e_d) * S))
// / 2e-9.  The fifteen estimates of a build pass (S and the fourteen stepped ones) and their inverses are the same for every edge: lanes 0..14 build them once
// per build pass into LDS, and an edge's Jacobian is fourteen plain projections.
//
// No edge keeps its error between passes (see mcs_poseopt.hip): whatever reads an edge's error reads the error of the CURRENT estimate.  The one
// per-correspondence state is its keep byte, cleared by the test behind round one.
#include "mcs_sim3opt.h"
#include "mcs_geom.h"
#include "mcs_sim3g.h"
#include "mcs_lm.h"

using namespace mcs;

namespace {

constexpr int kWaves = kSim3OptThreads / 64;
constexpr int kSums = 36;   // 28 of H (upper triangle, row-major), 7 of b, 1 of the robust chi2
constexpr int kEst = 15;    // S, then Sim3(+delta e_d) * S and Sim3(-delta e_d) * S for d = 0..6

struct Sim3Shared {
	OcamDev cam[32];
	double invMc[32][16];   // invMat(M_c[c])
	double MtInv[2][16];
	Sim3g E[kEst], Einv[kEst];   // [0]: the estimate the pass runs at
	double red[kWaves][kSums];
	double tot[kSums];
	double J[14][kSim3OptThreads];   // a thread's 2x7 Jacobian of the edge in hand, column by column: it is built in a rolled loop and read back unrolled
	double H[28], b[7];     // of the iteration's build pass (lane 0 reads them in every trial)
	Sim3g S, backup;
	double x[7];
	int nC, nonfinite, nBad, go, cont;
};

struct Corr { const double* Xw; const int* cam; const double* obs; const double* w; uint8_t* keep; int n; };

__device__ __forceinline__ bool pair_of(const Corr& e, int nr, int i, int& c1, int& c2) {
	c1 = e.cam[2 * i]; c2 = e.cam[2 * i + 1];
	return c1 >= 0 && c1 < nr && c2 >= 0 && c2 < nr;
}

// computeError of either edge class: obs - cam_map(S.map(P)) (include/g2o_MultiCol_sim3_expmap.h:141-161, 190-203, 224-238)
__device__ __forceinline__ void edge_error(const Sim3Shared& sh, const Sim3g& S, const double* P, int c, double ox, double oy, double& e0, double& e1) {
	double v[3], p[3], u, vv;
	sim3_map(S, P, v);
	matx44_point<3>(sh.invMc[c], v, p);
	omni_world_to_img(sh.cam[c], p[0], p[1], p[2], u, vv);
	e0 = ox - u; e1 = oy - vv;
}

// the estimates of a pass, from sh.S: Build: all fifteen and their inverses (lanes 0..14), else the estimate and its inverse (lane 0).  Barrier behind it.
template <bool Build>
__device__ void estimates(Sim3Shared& sh) {
	const int k = threadIdx.x;
	if (k < (Build ? kEst : 1)) {
		Sim3g E = sh.S;
		if (k > 0) {   // vi->oplus(add_vi) with add_vi[d] = +-delta (base_binary_edge.hpp:147-170): Sim3(update) * estimate
			const double delta = 1e-9;
			double u[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
			u[(k - 1) >> 1] = ((k - 1) & 1) ? -delta : delta;
			E = sim3_mul(sim3_exp(u), E);
		}
		sh.E[k] = E;
		sh.Einv[k] = sim3_inverse(E);
	}
	__syncthreads();
}

// One pass over the live correspondences at the estimates in sh.E / sh.Einv: the robust chi2 (activeRobustChi2), Build: also H and b
// (BaseBinaryEdge::constructQuadraticForm, the robust branch, core/base_binary_edge.hpp:91-113) with the numeric Jacobian.
template <bool Build>
__device__ void pass(Sim3Shared& sh, const Corr& e, int nr, double delta, double dsqr) {
	double acc[Build ? kSums : 1];
#pragma unroll
	for (int k = 0; k < (Build ? kSums : 1); ++k) acc[k] = 0.0;
	bool bad = false;
	for (int i = threadIdx.x; i < e.n; i += kSim3OptThreads) {
		int cc[2];
		if (!pair_of(e, nr, i, cc[0], cc[1]) || !e.keep[i]) continue;
		// the two edges: e12 maps the point of rig 2 with S, e21 the point of rig 1 with S^-1 (:113-146: invMat(M_t) * (Xw, 1))
#pragma unroll 1
		for (int g = 0; g < 2; ++g) {
			double P[3];
			matx44_point<3>(sh.MtInv[1 - g], e.Xw + 6 * (size_t)i + 3 * (1 - g), P);
			const Sim3g* Es = g == 0 ? sh.E : sh.Einv;
			const int c = cc[g];
			const double ox = e.obs[4 * (size_t)i + 2 * g], oy = e.obs[4 * (size_t)i + 2 * g + 1], w = e.w[2 * (size_t)i + g];
			double e0, e1;
			edge_error(sh, Es[0], P, c, ox, oy, e0, e1);
			const double c2 = e0 * (w * e0) + e1 * (w * e1);   // _error.dot(information() * _error)
			double rho0, rho1;
			huber_robustify(c2, delta, dsqr, rho0, rho1);
			if constexpr (!Build) { (void)rho1; acc[0] += rho0; }
			else {
			const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll 1
			for (int d = 0; d < 7; ++d) {   // rolled: two projections live at a time, not fourteen
				double p0, p1, m0, m1;
				edge_error(sh, Es[1 + 2 * d], P, c, ox, oy, p0, p1);
				edge_error(sh, Es[2 + 2 * d], P, c, ox, oy, m0, m1);
				const double j0 = scalar * (p0 - m0), j1 = scalar * (p1 - m1);
				sh.J[2 * d][threadIdx.x] = j0;
				sh.J[2 * d + 1][threadIdx.x] = j1;
				bad |= !finite_(j0) || !finite_(j1);
			}
			double J[2][7];
#pragma unroll
			for (int d = 0; d < 7; ++d) { J[0][d] = sh.J[2 * d][threadIdx.x]; J[1][d] = sh.J[2 * d + 1][threadIdx.x]; }
			bad |= !finite_(e0) || !finite_(e1) || !finite_(w);
			const double rw = rho1 * w;                                     // weightedOmega = rho[1] * information
			const double or0 = (-(w * e0)) * rho1, or1 = (-(w * e1)) * rho1;   // omega_r = -omega * _error; omega_r *= rho[1]
			int s = 0;
#pragma unroll
			for (int r = 0; r < 7; ++r)
#pragma unroll
				for (int q = r; q < 7; ++q) acc[s++] += (J[0][r] * rw) * J[0][q] + (J[1][r] * rw) * J[1][q];   // (B^T * weightedOmega) * B
#pragma unroll
			for (int r = 0; r < 7; ++r) acc[28 + r] += J[0][r] * or0 + J[1][r] * or1;   // B^T * omega_r
			acc[35] += rho0;
			}
		}
	}
	if (Build && bad) atomicOr(&sh.nonfinite, 1);
	block_sums<Build ? kSums : 1>(acc, sh.red, sh.tot);
}

// :206-226 / :241-257: a correspondence is bad if EITHER edge has chi2 > deltaHuber2, at the estimate in sh.E[0] / sh.Einv[0]
__device__ void outlier_pass(Sim3Shared& sh, const Corr& e, int nr, double dsqr) {
	int nbad = 0;
	for (int i = threadIdx.x; i < e.n; i += kSim3OptThreads) {
		int cc[2];
		if (!pair_of(e, nr, i, cc[0], cc[1]) || !e.keep[i]) continue;
		double chi[2];
#pragma unroll 1
		for (int g = 0; g < 2; ++g) {
			double P[3], e0, e1;
			matx44_point<3>(sh.MtInv[1 - g], e.Xw + 6 * (size_t)i + 3 * (1 - g), P);
			const double w = e.w[2 * (size_t)i + g];
			edge_error(sh, g == 0 ? sh.E[0] : sh.Einv[0], P, cc[g], e.obs[4 * (size_t)i + 2 * g], e.obs[4 * (size_t)i + 2 * g + 1], e0, e1);
			chi[g] = e0 * (w * e0) + e1 * (w * e1);
		}
		if (chi[0] > dsqr || chi[1] > dsqr) { e.keep[i] = 0; ++nbad; }
	}
	if (nbad) atomicAdd(&sh.nBad, nbad);
	__syncthreads();
}

__global__ void __launch_bounds__(kSim3OptThreads) k_sim3opt(Sim3OptArgs a, Sim3OptChunk ch, int first) {
	__shared__ Sim3Shared sh;
	const int tid = threadIdx.x, lp = blockIdx.x, gp = first + lp, nr = a.nrCams;
	const Corr e{ch.Xw[lp], ch.cam[lp], ch.obs[lp], ch.w[lp], ch.keep[lp], ch.n[lp]};

	if (tid < nr) {
		sh.cam[tid] = ocam_dev_of(a.cams[tid]);
		inv_mat(a.Mc + 16 * tid, sh.invMc[tid]);
	}
	if (tid >= 64 && tid < 96) sh.MtInv[(tid - 64) >> 4][tid & 15] = a.MtInv[32 * (size_t)gp + (tid - 64)];
	if (tid == 0) {
		sh.S = sim3_from_rts(a.R12 + 9 * (size_t)gp, a.t12 + 3 * (size_t)gp, a.s12[gp]);   // setEstimate(g2oS12), with Sim3(R, t, s) (sim3.h:64-67)
		for (int k = 0; k < 7; ++k) sh.x[k] = 0.0;
		sh.nC = 0; sh.nonfinite = 0; sh.nBad = 0;
	}
	int mine = 0;
	for (int i = tid; i < e.n; i += kSim3OptThreads) {
		int c1, c2;
		e.keep[i] = 1;
		mine += pair_of(e, nr, i, c1, c2) ? 1 : 0;
	}
	__syncthreads();
	if (mine) atomicAdd(&sh.nC, mine);
	__syncthreads();
	const int nC = sh.nC;
	const Sim3g Sin = sh.S;

	const double delta = 1.345 * a.stdSim[gp], dsqr = delta * delta;   // deltaHuber, deltaHuber2 (:109-110)
	// lane 0's state
	int status = MCS_SIM3OPT_OK, iters[2] = {0, 0}, stop[2] = {STOP_NOT_RUN, STOP_NOT_RUN}, trials[2][10] = {}, nBad1 = 0;
	LmState lm{};
	lm.lambda = -1.0; lm.ni = 2.0;
	bool stopFlag = false, returned0 = nC == 0;   // no correspondence: optimize() returns before its loop, then 0 - 0 < 3

	if (nC > 0) {   // uniform
		for (int rnd = 0; rnd < 2; ++rnd) {
			const int maxIt = rnd == 0 || nBad1 == 0 ? 5 : 10;   // optimize(5); nMoreIterations (:228-232)
			bool resultOk = true;
			int it = 0, why = stopFlag ? STOP_NOT_RUN : STOP_ITERATIONS;
			if (tid == 0) for (int k = 0; k < 7; ++k) sh.x[k] = 0.0;   // Solver::resize: zeros
			while (true) {
				if (tid == 0) sh.go = it < maxIt && !stopFlag && resultOk;
				__syncthreads();
				if (!sh.go) break;
				// ---- OptimizationAlgorithmLevenberg::solve(it)
				estimates<true>(sh);
				pass<true>(sh, e, nr, delta, dsqr);
				if (rnd == 0 && it == 0) {   // the screen of the first evaluation: every edge's residual, Jacobian and weight, the Huber pair, the sums
					bool nf = sh.nonfinite || !finite_(delta) || !finite_(dsqr);
					for (int k = 0; k < kSums; ++k) nf |= !finite_(sh.tot[k]);
					if (nf) { status = MCS_SIM3OPT_NONFINITE; break; }   // uniform: not optimised
				}
				lm_iter_begin(lm, sh.tot[35]);   // every thread: written by lane 0 alone, the iteration's values would stay live around the loop in the others
				lm.rho = 0.0;                    // solve()'s "double rho=0;", for the same reason: lm_trial writes it before anything reads it
				if (tid == 0) {
					for (int k = 0; k < 28; ++k) sh.H[k] = sh.tot[k];
					for (int k = 0; k < 7; ++k) sh.b[k] = sh.tot[28 + k];
					if (it == 0) lm_start(lm, lm_lambda_init(max_abs_diag<7>(sh.H, 0.0)));
				}
				while (true) {
					bool ok2 = true;
					if (tid == 0) {
						double x[7];
						for (int k = 0; k < 7; ++k) x[k] = sh.x[k];
						sh.backup = sh.S;   // push
						ok2 = ldlt_solve<7>(sh.H, lm.lambda, sh.b, x);
						for (int k = 0; k < 7; ++k) sh.x[k] = x[k];
						sh.S = sim3_mul(sim3_exp(x), sh.S);   // oplusImpl: Sim3(update) * estimate, with the stale x after a failed solve
					}
					__syncthreads();
					estimates<false>(sh);
					pass<false>(sh, e, nr, delta, dsqr);
					if (tid == 0) {
						const double rawChi = sh.tot[0];
						double scale = 0.0;   // computeScale: the seven of x and b
						for (int j = 0; j < 7; ++j) scale += sh.x[j] * (lm.lambda * sh.x[j] + sh.b[j]);
						if (lm_trial(lm, rawChi, ok2, scale)) lm.postChi = rawChi;   // an accepted trial's pass evaluated the estimate the action will judge
						else sh.S = sh.backup;   // pop
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
			if (status != MCS_SIM3OPT_OK) break;
			iters[rnd] = it; stop[rnd] = why;
			// ---- the test behind this round, at the current estimate
			__syncthreads();
			estimates<false>(sh);
			outlier_pass(sh, e, nr, dsqr);
			if (rnd == 0) {
				nBad1 = sh.nBad;
				if (nC - nBad1 < 3) { returned0 = true; break; }   // :234-235: return 0 before g2oS12 is written; the matches stay nulled
			}
		}
	}
	__syncthreads();
	if (tid == 0) {   // a non-finite problem left the screen before any keep byte was cleared
		const Sim3g So = status == MCS_SIM3OPT_OK && !returned0 ? sh.S : Sin;
		sim3_store(So, a.S12 + 8 * (size_t)gp);
		if (a.R12out) quat_to_mat(So.q, a.R12out + 9 * (size_t)gp);
		a.nInliers[gp] = status != MCS_SIM3OPT_OK ? nC : returned0 ? 0 : nC - sh.nBad;
		if (a.diag) {
			mcs_sim3opt_diag& g = a.diag[gp];
			g.status = status; g.n_corr = nC; g.n_bad1 = status == MCS_SIM3OPT_OK ? nBad1 : 0; g.pad = 0;
			for (int r = 0; r < 2; ++r) { g.iters[r] = iters[r]; g.stop[r] = stop[r]; for (int k = 0; k < 10; ++k) g.trials[r][k] = trials[r][k]; }
			g.lambda = nC > 0 && status == MCS_SIM3OPT_OK ? lm.lambda : 0.0; g.chi2 = status == MCS_SIM3OPT_OK ? lm.lastChi : 0.0;
		}
	}
}

}  // namespace

namespace mcs {
void launch_sim3opt(const Sim3OptArgs& a, const Sim3OptChunk& ch, int first, int count, hipStream_t s) {
	hipLaunchKernelGGL(k_sim3opt, dim3(count), dim3(kSim3OptThreads), 0, s, a, ch, first);
}
}  // namespace mcs

// ---------------------------------------------------------------------------------------------- cOptimizer::OptimizeSim3
int mcs_sim3_optimize(mcs_ctx* c, int nproblems, const mcs_sim3opt_problem* problems, const double* M_c, const mcs_ocam* cams, int nr_cams,
                      const double* M_t_inv, const double* std_sim, const double* R12, const double* t12, const double* s12, mcs_mem_kind kind, double* S12,
                      double* R12_out, uint8_t* const* keep, int32_t* n_inliers, mcs_sim3opt_diag* diag) {
	const Sim3OptCall q{nproblems, problems, M_c, cams, nr_cams, M_t_inv, std_sim, R12, t12, s12, kind, S12, R12_out, keep, n_inliers, diag};
	if (int r = guard_sim3opt(c, q, c && c->asyncSearch)) return r;
	if (nproblems == 0) return MCS_OK;
	const bool host = kind == MCS_MEM_HOST;
	if (host)
		if (int r = guard_sim3opt_content(q)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (int r = ctx_join_greedy(c, s)) return r;   // the matches may come from a search whose greedy pass runs on the side stream
	const size_t np = nproblems, nr = nr_cams;
	Sim3OptArgs a{};
	a.nrCams = nr_cams;
	std::vector<const double*> Xw(np), obs(np), w(np); std::vector<const int*> cam(np); std::vector<uint8_t*> out(np);
	Staging st(c, host);
	st.in(&a.Mc, M_c, nr * 128); st.in(&a.cams, cams, nr * sizeof(mcs_ocam)); st.in(&a.MtInv, M_t_inv, np * 256); st.in(&a.stdSim, std_sim, np * 8);
	st.in(&a.R12, R12, np * 72); st.in(&a.t12, t12, np * 24); st.in(&a.s12, s12, np * 8);
	st.out(&a.S12, S12, np * 64);
	if (R12_out) st.out(&a.R12out, R12_out, np * 72);
	st.out(&a.nInliers, n_inliers, np * 4);
	if (diag) st.out(&a.diag, diag, np * sizeof(mcs_sim3opt_diag));
	for (size_t p = 0; p < np; ++p) {
		const size_t n = problems[p].n;
		st.in(&Xw[p], problems[p].Xw, n * 48); st.in(&cam[p], problems[p].cam, n * 8); st.in(&obs[p], problems[p].obs, n * 32); st.in(&w[p], problems[p].w, n * 16);
		if (n) st.out(&out[p], keep[p], n); else out[p] = nullptr;
	}
	if (int r = st.commit()) return r;
	c->tic("sim3_optimize");
	for (int first = 0; first < nproblems; first += kSim3OptBatch) {
		const int count = std::min(kSim3OptBatch, nproblems - first);
		Sim3OptChunk ch{};
		for (int k = 0; k < count; ++k) {
			ch.Xw[k] = Xw[first + k]; ch.cam[k] = cam[first + k]; ch.obs[k] = obs[first + k]; ch.w[k] = w[first + k]; ch.keep[k] = out[first + k];
			ch.n[k] = problems[first + k].n;
		}
		launch_sim3opt(a, ch, first, count, s);
	}
	c->toc("sim3_optimize");
	c->lastResultStream = s;   // every output is complete on the context's stream
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}
