// mcs_lm.h — what the four device optimisers (mcs_poseopt / mcs_sim3opt / mcs_lba / mcs_essgraph.hip) share, stated once: g2o's Levenberg-Marquardt loop
// as plain functions over one small state, its Huber kernel, the small unpivoted LDL^T, the ordered reductions and the ordered compaction.  Each function
// restates the cited lines of ThirdParty/g2o/g2o/core and keeps their operation order: FP64, no contraction.  What differs between the four call sites
// (computeScale's terms, when postChi is written, the stop flag, the iteration cap, the first lambda, the chi2 reported) stays at the call site.  The host
// side — everything but the wave and workgroup primitives — is held bit for bit to tests/poseopt_model.py and tests/essgraph_model.py by
// tests/test_lm_cpu.py, which compiles this header alone for the host (tests/cpp/lm_driver.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <cfloat>

#ifndef MCS_GEOM
#define MCS_GEOM __host__ __device__ __forceinline__
#endif

namespace mcs {

// why a run of iterations ended: all of them ran; the terminate action set the stop flag; solve() returned Terminate after 10 trials or with rho == 0;
// solve() returned Terminate by the nBad >= 3 rule; it never started; the action's iteration cap (the essential graph alone).  The values are in the
// diag structs of include/mcs_c.h.
enum { STOP_ITERATIONS = 0, STOP_GAIN = 1, STOP_TRIALS = 2, STOP_NBAD = 3, STOP_NOT_RUN = 4, STOP_CAP = 5 };

// g2o_isfinite (stuff/macros.h): false for a NaN and for either infinity
MCS_GEOM bool finite_(double v) { return fabs(v) <= DBL_MAX; }

// RobustKernelHuber::robustify (core/robust_kernel_impl.cpp:78-91): rho[0] and rho[1]; no caller reads the second-order term
MCS_GEOM void huber_robustify(double c2, double delta, double dsqr, double& rho0, double& rho1) {
	if (c2 <= dsqr) { rho0 = c2; rho1 = 1.0; }
	else { const double sq = sqrt(c2); rho0 = 2 * sq * delta - dsqr; rho1 = delta / sq; }
}

// unpivoted LDL^T of H + lambda I (H: upper triangle, row-major) and the solve; false as soon as a pivot is not > 0 (x is then left alone).  The
// project's replacement for the reference's linear solver.  One call, not inlined: lane 0 of a 256-VGPR kernel runs it.
template <int N>
__host__ __device__ __noinline__ bool ldlt_solve(const double* Hu, double lambda, const double* b, double* x) {
	double A[N][N], L[N][N], d[N], y[N];
	int s = 0;
#pragma unroll
	for (int r = 0; r < N; ++r)
#pragma unroll
		for (int q = r; q < N; ++q) { A[r][q] = A[q][r] = Hu[s++]; }
#pragma unroll
	for (int r = 0; r < N; ++r) A[r][r] = A[r][r] + lambda;
#pragma unroll
	for (int j = 0; j < N; ++j) {
		double t = A[j][j];
#pragma unroll
		for (int k = 0; k < j; ++k) t -= L[j][k] * L[j][k] * d[k];
		if (!(t > 0.0)) return false;
		d[j] = t;
#pragma unroll
		for (int i = j + 1; i < N; ++i) {
			double u = A[i][j];
#pragma unroll
			for (int k = 0; k < j; ++k) u -= L[i][k] * L[j][k] * d[k];
			L[i][j] = u / t;
		}
	}
#pragma unroll
	for (int i = 0; i < N; ++i) {
		double t = b[i];
#pragma unroll
		for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
		y[i] = t;
	}
#pragma unroll
	for (int i = 0; i < N; ++i) y[i] = y[i] / d[i];
#pragma unroll
	for (int i = N - 1; i >= 0; --i) {
		double t = y[i];
#pragma unroll
		for (int k = i + 1; k < N; ++k) t -= L[k][i] * x[k];
		x[i] = t;
	}
	return true;
}

// ---------------------------------------------------------------------------------------------- OptimizationAlgorithmLevenberg and the terminate action
// _currentLambda, _ni, solve()'s locals, _levenbergIterations and _nBad (core/optimization_algorithm_levenberg.cpp:82-101); postChi is the chi2 of the
// evaluation the edges' errors come from when the terminate action reads them, lastChi the action's _lastChi
struct LmState { double lambda, ni, currentChi, iniChi, postChi, lastChi, rho; int qmax, lmBad; };

// the largest |H_jj| of an NxN block kept as its upper triangle, row-major, folded into m (computeLambdaInit's loop, :170-178)
template <int N>
MCS_GEOM double max_abs_diag(const double* Hu, double m) {
	int s = 0;
	for (int r = 0; r < N; ++r) { m = fmax(fabs(Hu[s]), m); s += N - r; }
	return m;
}
// computeLambdaInit without a user value (:170-179): tau * max |H_jj|, tau = 1e-5
MCS_GEOM double lm_lambda_init(double maxDiag) { return 1e-5 * maxDiag; }

// solve(iteration == 0), :93-97, with the lambda the caller computed
MCS_GEOM void lm_start(LmState& s, double lambda) { s.lambda = lambda; s.ni = 2.0; s.lmBad = 0; }
// solve(), :82-85 and :99-101, with the robust chi2 of the build pass
MCS_GEOM void lm_iter_begin(LmState& s, double chi) { s.currentChi = s.iniChi = s.postChi = chi; s.qmax = 0; }

// One trial, :124-148, behind the evaluation of the trial estimate: rawChi is its robust chi2, solveOk what the linear solver returned, scale the caller's
// computeScale().  True: the step was accepted (discardTop), false: the caller restores (pop).  postChi is the caller's to write.
MCS_GEOM bool lm_trial(LmState& s, double rawChi, bool solveOk, double scale) {
	const double tempChi = solveOk ? rawChi : DBL_MAX;
	double rho = s.currentChi - tempChi;
	scale += 1e-3;
	rho /= scale;
	const bool accepted = rho > 0 && finite_(tempChi);
	if (accepted) {
		double alpha = 1. - pow(2 * rho - 1, 3.0);
		alpha = fmin(alpha, 2. / 3.);
		s.lambda *= fmax(1. / 3., alpha);
		s.ni = 2;
		s.currentChi = tempChi;
	} else {
		s.lambda *= s.ni;
		s.ni *= 2;
	}
	++s.qmax;
	s.rho = rho;
	return accepted;
}
// the trial loop's condition, :149, without the optimiser's stop flag (the caller's term)
MCS_GEOM bool lm_more(const LmState& s) { return s.rho < 0 && s.qmax < 10; }

// solve()'s return behind the trial loop, :151-163: STOP_ITERATIONS for OK, else the Terminate that fired
MCS_GEOM int lm_iter_end(LmState& s) {
	if (s.qmax == 10 || s.rho == 0) return STOP_TRIALS;
	s.lmBad = (s.iniChi - s.currentChi) * 1e3 < s.iniChi ? s.lmBad + 1 : 0;
	return s.lmBad >= 3 ? STOP_NBAD : STOP_ITERATIONS;
}
// SparseOptimizerTerminateAction::operator() (core/sparse_optimizer_terminate_action.cpp:24-57) below its iteration cap, on postChi: iteration 0 stores
// the chi2, a later one tests the gain against 1e-6.  True: the action sets the optimiser's stop flag.
MCS_GEOM bool lm_gain_stop(LmState& s, int it) {
	if (it == 0) { s.lastChi = s.postChi; return false; }
	const double gain = (s.lastChi - s.postChi) / s.postChi;
	s.lastChi = s.postChi;
	return gain >= 0 && gain < 1e-6;
}

// ---------------------------------------------------------------------------------------------- ordered sums and ordered lists
inline dim3 blocks(size_t n, int per) { return dim3((unsigned)std::max<size_t>(1, (n + per - 1) / per)); }

// acc[0..N) over the 64 lanes by a fixed shuffle tree: lane 0 holds the sums
template <int N>
__device__ __forceinline__ void wave_sum(double* acc) {
#pragma unroll
	for (int k = 0; k < N; ++k) {
		double v = acc[k];
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
		acc[k] = v;
	}
}
// ... over a workgroup of Waves waves: wave_sum, then the waves in ascending order; tot[0..N) on every thread after the closing barrier
template <int N, int Waves, int Stride>
__device__ __forceinline__ void block_sums(double* acc, double (&red)[Waves][Stride], double* tot) {
	static_assert(N <= Stride, "a wave's row holds the N sums");
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	wave_sum<N>(acc);
	if (lane == 0) {
#pragma unroll
		for (int k = 0; k < N; ++k) red[wave][k] = acc[k];
	}
	__syncthreads();
	if (threadIdx.x < N) {
		double t = red[0][threadIdx.x];
		for (int w = 1; w < Waves; ++w) t += red[w][threadIdx.x];
		tot[threadIdx.x] = t;
	}
	__syncthreads();
}

// the indices of [0, n) that satisfy pred, in ascending order, by a workgroup of Threads: returns their number on every thread; Fill: also writes them to
// out (a ballot per wave, the waves' counts through LDS).  Every thread of the workgroup calls it; the kernel's __launch_bounds__ is Threads.
template <bool Fill, int Threads, class Pred>
__device__ __forceinline__ int compact_indices(int n, Pred pred, int* out) {
	static_assert(Threads % 64 == 0, "whole waves");
	constexpr int Waves = Threads / 64;
	__shared__ int wc[Waves];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int running = 0;
	for (int base = 0; base < n; base += Threads) {
		const int e = base + threadIdx.x;
		const bool m = e < n && pred(e);
		const unsigned long long bal = __ballot(m);
		if (lane == 0) wc[wave] = __popcll(bal);
		__syncthreads();
		int before = 0, all = 0;
		for (int w = 0; w < Waves; ++w) { if (w < wave) before += wc[w]; all += wc[w]; }
		if (Fill && m) out[running + before + __popcll(bal & ((1ull << lane) - 1ull))] = e;
		running += all;
		__syncthreads();
	}
	return running;
}
// where each of n counted lists starts, and in off[n] their total: one thread
__device__ __forceinline__ void list_offsets(const int* count, int* off, int n) {
	int at = 0;
	for (int f = 0; f < n; ++f) { off[f] = at; at += count[f]; }
	off[n] = at;
}

}  // namespace mcs
