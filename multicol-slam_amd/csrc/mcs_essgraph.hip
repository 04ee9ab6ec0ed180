// mcs_essgraph.hip — cOptimizer::OptimizeEssentialGraph (src/cOptimizerLoopStuff.cpp:267-513) as one problem over the whole device, and the entry point
// mcs_optimize_essential_graph (include/mcs_c.h).  DESIGN.md 4o; the statement-by-statement restatement the kernels are held to is tests/essgraph_model.py.
// The Levenberg-Marquardt steps, the wave sums and the ordered lists are csrc/mcs_lm.h's, the Sim3 arithmetic csrc/mcs_sim3g.h's.
//
// The phases are separate launches on the context's stream — no grid-wide barrier, no workgroup waits for another inside a launch:
//   k_eg_prepare       per edge: the guards, the measurement Sjw * Swi from Scw / Snc
//   k_eg_lists         per free vertex: its incident edges in ascending order (count, then fill), once per call
//   k_eg_vertices      per (vertex, evaluation): S and Sim3(+-1e-9 e_d) S, and their inverses — shared by every edge at that vertex
//   k_eg_linearise     per (edge, evaluation): the 29 residuals log(C Si Sj^-1), then both 7x7 numeric Jacobians, the residual and chi2 of the edge
//   k_eg_residuals     per edge: the residual and chi2 at the trial estimates
//   k_eg_reduce        one workgroup: chi2 over the edges and the terms of computeScale over x, thread-strided in ascending order, then a fixed tree
//   k_eg_iter_begin    one thread: currentChi, the screen of the first evaluation, lambda = 1e-6 at iteration 0
//   k_eg_assemble      one wave per free vertex i: walks its list in ascending order and owns block row i of the dense lower triangle of H + lambda I, and b_i
//   k_eg_factor        one workgroup: the unpivoted LDL^T of a panel's diagonal block
//   k_eg_panel         a thread per row below it: the panel's L
//   k_eg_trail         a workgroup per 64 x 64 tile of the trailing lower triangle: minus the panel's L D L^T
//   k_eg_subst         one workgroup: both substitutions in panels, x
//   k_eg_apply         per vertex: the trial estimate Sim3(x_i) * S_i
//   k_eg_decide        one thread: rho, lambda / ni, accept or restore, the trial count, solve()'s return, the terminate action; the 64-byte record
//   k_eg_accept        the trial estimates become the estimates where the trial was accepted
//   k_eg_writeback     Scw_out, pose, kf_t per vertex; pos per map point
// Every decision that depends on arithmetic is taken on the device; the host loop reads the record after ONE stream synchronisation per trial.
//
// The solve.  Column j of an unpivoted LDL^T divides the column by d_j and takes (l_rj * l_kj) * d_j from every entry (r, k) behind it.  The blocked form
// here applies exactly these subtractions to every entry in increasing j — inside the diagonal block (k_eg_factor), in the panel solve (k_eg_panel) and in
// the trailing update (k_eg_trail) — so the factor is the one the column-by-column loop of k_lba_solve would give, bit for bit, whatever the tiling.  The
// substitutions subtract in increasing k (forward) and decreasing k (backward) per unknown.  It fails at the first pivot that is zero or not finite.
#include "mcs_essgraph.h"
#include "mcs_geom.h"
#include "mcs_sim3g.h"
#include "mcs_lm.h"

using namespace mcs;

namespace {

constexpr int kEdgeDoubles = 49 + 49 + 7 + 1;   // A [7][7] (row: residual component, column: d), B, e, chi2
constexpr int NB = kEgPanel;
constexpr int kMaxN = 7 * kEgMaxFree;

struct EgCtl {   // the Levenberg-Marquardt state, on the device
	LmState lm;
	double sumChi, sumScale;   // of k_eg_reduce
	int nonfinite, solveOk, accepted, nEdgesOk;
};
struct EgRecord {   // 64 bytes, page-locked host memory: what the host loop reads
	int more, resultOk, why, stopNow, qmax, nonfinite, nEdgesOk, accepted;
	double lambda, chi2;
	int pad[4];
};
static_assert(sizeof(EgRecord) == 64, "the control record is 64 bytes");

struct EgDev {
	int nKfs, nEdges, nPoints, nFree, N;
	const double* Scw; const double* Snc; const uint8_t* hasNc; const int* edgeI; const int* edgeJ; const uint8_t* edgeKind; double* posIO; const int* ptRef;
	double* ScwOut; double* poseOut; double* kfT;
	const int* fidx; const int* freeKf;   // [nKfs] free index or -1, [nFree] vertex of a free index
	double* est; double* estT;            // [nKfs][8]
	double* V; double* Vinv;              // [nKfs][15][8]
	uint8_t* ok; double* meas;            // per edge: passed the guards; Sjw * Swi [8]
	double* edge; double* eChi;           // [nEdges][kEdgeDoubles]; [nEdges] chi2 of the latest evaluation
	int* vCount; int* vOff; int* vList;   // [nFree], [nFree + 1], [2 nEdges]
	double* S; double* dd; double* b; double* x;   // [N][N] (lower triangle), [N], [N], [N]
	EgCtl* ctl; EgRecord* rec;
};

// ---------------------------------------------------------------------------------------------- once per call
__global__ void k_eg_prepare(EgDev d) {
	const int e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= d.nEdges) return;
	const int i = d.edgeI[e], j = d.edgeJ[e];
	const bool ok = i >= 0 && i < d.nKfs && j >= 0 && j < d.nKfs && i != j;
	d.ok[e] = ok;
	if (!ok) return;
	const bool nc = d.edgeKind[e] != 0;
	const Sim3g Siw = sim3_load((nc && d.hasNc[i] ? d.Snc : d.Scw) + 8 * (size_t)i);
	const Sim3g Sjw = sim3_load((nc && d.hasNc[j] ? d.Snc : d.Scw) + 8 * (size_t)j);
	sim3_store(sim3_mul(Sjw, sim3_inverse(Siw)), d.meas + 8 * (size_t)e);
	atomicAdd(&d.ctl->nEdgesOk, 1);
}

// the edges at free vertex blockIdx.x in ascending order: Fill = false counts, Fill = true writes behind vOff
template <bool Fill>
__global__ void __launch_bounds__(256) k_eg_lists(EgDev d) {
	const int f = blockIdx.x, v = d.freeKf[f];
	const int n = compact_indices<Fill, 256>(d.nEdges, [&](int e) { return d.ok[e] && (d.edgeI[e] == v || d.edgeJ[e] == v); }, Fill ? d.vList + d.vOff[f] : nullptr);
	if (!Fill && threadIdx.x == 0) d.vCount[f] = n;
}

__global__ void k_eg_offsets(EgDev d) {
	if (blockIdx.x || threadIdx.x) return;
	list_offsets(d.vCount, d.vOff, d.nFree);
	EgRecord r{};
	r.nEdgesOk = d.ctl->nEdgesOk;
	*d.rec = r;
}

// ---------------------------------------------------------------------------------------------- an evaluation
// evaluation k of vertex v at `est`: 0 the estimate, 1 + 2d / 2 + 2d the estimate moved by Sim3(+-1e-9 e_d) (oplusImpl: Sim3(update) * estimate), and the inverse
__global__ void k_eg_vertices(EgDev d, const double* est, int nEval) {
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= d.nKfs * nEval) return;
	const int v = t / nEval, k = t - v * nEval;
	Sim3g S = sim3_load(est + 8 * (size_t)v);
	if (k > 0) {
		double u[7] = {0, 0, 0, 0, 0, 0, 0};
		u[(k - 1) >> 1] = (k & 1) ? 1e-9 : -1e-9;
		S = sim3_mul(sim3_exp(u), S);
	}
	sim3_store(S, d.V + 8 * ((size_t)v * 15 + k));
	sim3_store(sim3_inverse(S), d.Vinv + 8 * ((size_t)v * 15 + k));
}

// Two edges per workgroup of 64, 32 lanes each, 29 of them at work: evaluation 0 is the residual, 1..14 move vertex i, 15..28 vertex j
// (base_binary_edge.hpp:130-205).  Then the lanes share out the 98 Jacobian entries: column d = (e(+) - e(-)) * (1 / 2e-9).
__global__ void __launch_bounds__(64) k_eg_linearise(EgDev d) {
	__shared__ double r[2][29][7];
	const int half = threadIdx.x >> 5, lane = threadIdx.x & 31, e = blockIdx.x * 2 + half;
	const bool live = e < d.nEdges && d.ok[e];
	int i = 0, j = 0;
	if (live) { i = d.edgeI[e]; j = d.edgeJ[e]; }
	if (live && lane < 29) {
		const int ki = lane < 15 ? lane : 0, kj = lane < 15 ? 0 : lane - 14;
		double out[7];
		sim3_edge_error(sim3_load(d.meas + 8 * (size_t)e), sim3_load(d.V + 8 * ((size_t)i * 15 + ki)), sim3_load(d.Vinv + 8 * ((size_t)j * 15 + kj)), out);
#pragma unroll
		for (int k = 0; k < 7; ++k) r[half][lane][k] = out[k];
	}
	__syncthreads();
	if (!live) { if (e < d.nEdges && lane == 0) d.eChi[e] = 0.0; return; }
	double* o = d.edge + (size_t)e * kEdgeDoubles;
	const double scalar = 1.0 / (2 * 1e-9);
	const bool freeI = d.fidx[i] >= 0, freeJ = d.fidx[j] >= 0;
	bool bad = false;
	for (int q = lane; q < 98; q += 32) {
		const int side = q / 49, rc = q - 49 * side, row = rc / 7, col = rc - 7 * row;
		const int base = side ? 15 : 1;
		const double v = scalar * (r[half][base + 2 * col][row] - r[half][base + 2 * col + 1][row]);
		o[q] = v;
		if (side ? freeJ : freeI) bad |= !finite_(v);
	}
	if (lane < 7) { o[98 + lane] = r[half][0][lane]; bad |= !finite_(r[half][0][lane]); }
	if (lane == 0) {
		double c = r[half][0][0] * r[half][0][0];   // _error.dot(information() * _error) with the identity
#pragma unroll
		for (int k = 1; k < 7; ++k) c += r[half][0][k] * r[half][0][k];
		o[105] = c;
		d.eChi[e] = c;
	}
	if (bad) atomicOr(&d.ctl->nonfinite, 1);
}

__global__ void k_eg_residuals(EgDev d) {
	const int e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= d.nEdges) return;
	if (!d.ok[e]) { d.eChi[e] = 0.0; return; }
	double r[7];
	sim3_edge_error(sim3_load(d.meas + 8 * (size_t)e), sim3_load(d.V + 8 * (size_t)d.edgeI[e] * 15), sim3_load(d.Vinv + 8 * (size_t)d.edgeJ[e] * 15), r);
	double c = r[0] * r[0];
#pragma unroll
	for (int k = 1; k < 7; ++k) c += r[k] * r[k];
	d.eChi[e] = c;
}

// one workgroup: chi2 over the edges and (trial) x_k (lambda x_k + b_k) over the unknowns, thread-strided in ascending order, the shuffle tree, the waves in order
__global__ void __launch_bounds__(1024) k_eg_reduce(EgDev d, int trial) {
	__shared__ double red[16][2];
	double acc[2] = {0.0, 0.0};
	for (int e = threadIdx.x; e < d.nEdges; e += 1024) acc[0] += d.eChi[e];
	if (trial) {
		const double lam = d.ctl->lm.lambda;
		for (int k = threadIdx.x; k < d.N; k += 1024) acc[1] += d.x[k] * (lam * d.x[k] + d.b[k]);
	}
	wave_sum<2>(acc);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (lane == 0) { red[wave][0] = acc[0]; red[wave][1] = acc[1]; }
	__syncthreads();
	if (threadIdx.x == 0) {
		double s0 = red[0][0], s1 = red[0][1];
		for (int w = 1; w < 16; ++w) { s0 += red[w][0]; s1 += red[w][1]; }
		d.ctl->sumChi = s0;
		if (trial) d.ctl->sumScale = s1;
	}
}

__global__ void k_eg_iter_begin(EgDev d, int it) {
	if (blockIdx.x || threadIdx.x) return;
	EgCtl& c = *d.ctl;
	lm_iter_begin(c.lm, c.sumChi);
	if (it == 0) {
		if (!finite_(c.sumChi)) c.nonfinite = 1;
		lm_start(c.lm, 1e-6);   // not lm_lambda_init: computeLambdaInit returns the user's value (optimization_algorithm_levenberg.cpp:168-169)
	}
}

// ---------------------------------------------------------------------------------------------- a trial
// One wave per free vertex f.  Lanes 0..48 hold entry (r, c) of a 7x7 block, lanes 49..55 an entry of b_f.  The diagonal block and b_f are summed over the
// vertex's edges in ascending order and written once (plus lambda on the diagonal); the block towards a free neighbour g < f is added into S, which was
// zeroed: this wave is the only writer of block row f, and parallel edges add up in edge order.  The sums over the seven residual rows run in increasing k.
__global__ void __launch_bounds__(64) k_eg_assemble(EgDev d) {
	const int f = blockIdx.x, v = d.freeKf[f], lane = threadIdx.x, n = d.vCount[f];
	const int* list = d.vList + d.vOff[f];
	const int r = lane / 7, c = lane - 7 * r;   // lanes 0..48
	double acc = 0.0;
	for (int t = 0; t < n; ++t) {
		const int e = list[t];
		const bool isI = d.edgeI[e] == v;
		const double* o = d.edge + (size_t)e * kEdgeDoubles;
		const double* own = isI ? o : o + 49;
		const double* oth = isI ? o + 49 : o;
		if (lane < 49) {
			double s = own[r] * own[c];
#pragma unroll
			for (int k = 1; k < 7; ++k) s += own[7 * k + r] * own[7 * k + c];
			acc += s;
		} else if (lane < 56) {
			const int q = lane - 49;
			double s = own[q] * -o[98];
#pragma unroll
			for (int k = 1; k < 7; ++k) s += own[7 * k + q] * -o[98 + k];
			acc += s;
		}
		const int g = d.fidx[isI ? d.edgeJ[e] : d.edgeI[e]];
		if (g >= 0 && g < f && lane < 49) {
			double s = own[r] * oth[c];
#pragma unroll
			for (int k = 1; k < 7; ++k) s += own[7 * k + r] * oth[7 * k + c];
			d.S[(size_t)(7 * f + r) * d.N + 7 * g + c] += s;
		}
	}
	if (lane < 49) { if (c <= r) d.S[(size_t)(7 * f + r) * d.N + 7 * f + c] = acc + (r == c ? d.ctl->lm.lambda : 0.0); }
	else if (lane < 56) d.b[7 * f + lane - 49] = acc;
	if (f == 0 && lane == 0) d.ctl->solveOk = 1;
}

// the diagonal block [c0, c0 + nb) of the panel: column by column, in shared memory; d_j to dd, the unit-lower factor back into S
__global__ void __launch_bounds__(1024) k_eg_factor(EgDev d, int c0, int nb) {
	__shared__ double A[NB][NB + 1];
	if (!d.ctl->solveOk) return;
	const int r = threadIdx.x >> 5, k = threadIdx.x & 31;
	const bool in = r < nb && k <= r;
	A[r][k] = in ? d.S[(size_t)(c0 + r) * d.N + c0 + k] : 0.0;
	__syncthreads();
	for (int j = 0; j < nb; ++j) {
		const double dj = A[j][j];
		if (dj == 0.0 || !finite_(dj)) {   // uniform
			if (threadIdx.x == 0) d.ctl->solveOk = 0;
			return;
		}
		if (k == j && r > j && r < nb) A[r][j] = A[r][j] / dj;
		__syncthreads();
		if (r > j && r < nb && k > j && k <= r) A[r][k] -= (A[r][j] * A[k][j]) * dj;
		__syncthreads();
	}
	if (r < nb && k < r) d.S[(size_t)(c0 + r) * d.N + c0 + k] = A[r][k];
	if (r < nb && k == r) d.dd[c0 + r] = A[r][r];
}

// a thread per row below a full panel: l_rc = (a_rc - sum_{k < c} (l_rk * L_ck) * d_k) / d_c, the subtractions in increasing k
__global__ void __launch_bounds__(64) k_eg_panel(EgDev d, int c0) {
	__shared__ double L[NB][NB + 1], dj[NB];
	if (!d.ctl->solveOk) return;
	for (int t = threadIdx.x; t < NB * NB; t += 64) { const int r = t >> 5, k = t & 31; L[r][k] = k < r ? d.S[(size_t)(c0 + r) * d.N + c0 + k] : 0.0; }
	if (threadIdx.x < NB) dj[threadIdx.x] = d.dd[c0 + threadIdx.x];
	__syncthreads();
	const int row = c0 + NB + blockIdx.x * 64 + threadIdx.x;
	if (row >= d.N) return;
	double* p = d.S + (size_t)row * d.N + c0;
	double a[NB];
#pragma unroll
	for (int c = 0; c < NB; ++c) a[c] = p[c];
#pragma unroll
	for (int c = 0; c < NB; ++c) {
		double s = a[c];
#pragma unroll
		for (int k = 0; k < c; ++k) s -= (a[k] * L[c][k]) * dj[k];
		a[c] = s / dj[c];
	}
#pragma unroll
	for (int c = 0; c < NB; ++c) p[c] = a[c];
}

// a workgroup per 64 x 64 tile (blockIdx.y >= blockIdx.x) of the lower triangle behind a full panel: s_rk -= (l_rj * l_kj) * d_j for j = 0..31 in order
__global__ void __launch_bounds__(256) k_eg_trail(EgDev d, int c0) {
	if (blockIdx.x > blockIdx.y) return;
	__shared__ double Lr[64][NB + 1], Lk[64][NB + 1], dj[NB];
	if (!d.ctl->solveOk) return;
	const int c1 = c0 + NB, r0 = c1 + 64 * blockIdx.y, k0 = c1 + 64 * blockIdx.x, N = d.N;
	for (int t = threadIdx.x; t < 64 * NB; t += 256) {
		const int r = t >> 5, k = t & 31;
		Lr[r][k] = r0 + r < N ? d.S[(size_t)(r0 + r) * N + c0 + k] : 0.0;
		Lk[r][k] = k0 + r < N ? d.S[(size_t)(k0 + r) * N + c0 + k] : 0.0;
	}
	if (threadIdx.x < NB) dj[threadIdx.x] = d.dd[c0 + threadIdx.x];
	__syncthreads();
	const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
	double acc[4][4];
#pragma unroll
	for (int a = 0; a < 4; ++a)
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const int r = r0 + ty + 16 * a, k = k0 + tx + 16 * b;
			acc[a][b] = r < N && k <= r ? d.S[(size_t)r * N + k] : 0.0;
		}
	for (int j = 0; j < NB; ++j) {
		const double dv = dj[j];
		double lr[4], lk[4];
#pragma unroll
		for (int a = 0; a < 4; ++a) { lr[a] = Lr[ty + 16 * a][j]; lk[a] = Lk[tx + 16 * a][j]; }
#pragma unroll
		for (int a = 0; a < 4; ++a)
#pragma unroll
			for (int b = 0; b < 4; ++b) acc[a][b] -= (lr[a] * lk[b]) * dv;
	}
#pragma unroll
	for (int a = 0; a < 4; ++a)
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const int r = r0 + ty + 16 * a, k = k0 + tx + 16 * b;
			if (r < N && k <= r) d.S[(size_t)r * N + k] = acc[a][b];
		}
}

// one workgroup: L y = b panel by panel (inside the diagonal block from shared memory, then every row below takes the panel's 32 terms in increasing k),
// y / d, L^T x = y from the last panel to the first (every row above takes the panel's terms in decreasing k).  After a failed factorisation x stays.
__global__ void __launch_bounds__(1024) k_eg_subst(EgDev d) {
	__shared__ double y[kMaxN], L[NB][NB + 1];
	if (!d.ctl->solveOk) return;
	const int N = d.N, tid = threadIdx.x;
	const double* S = d.S;
	for (int r = tid; r < N; r += 1024) y[r] = d.b[r];
	__syncthreads();
	for (int c0 = 0; c0 < N; c0 += NB) {
		const int nb = min(NB, N - c0), c1 = c0 + nb;
		{ const int r = tid >> 5, k = tid & 31; L[r][k] = r < nb && k < r ? S[(size_t)(c0 + r) * N + c0 + k] : 0.0; }
		__syncthreads();
		for (int k = 0; k < nb; ++k) {
			if (tid > k && tid < nb) y[c0 + tid] -= L[tid][k] * y[c0 + k];
			__syncthreads();
		}
		for (int r = c1 + tid; r < N; r += 1024) {
			const double* p = S + (size_t)r * N + c0;
			double s = y[r];
			for (int k = 0; k < nb; ++k) s -= p[k] * y[c0 + k];
			y[r] = s;
		}
		__syncthreads();
	}
	for (int r = tid; r < N; r += 1024) y[r] = y[r] / d.dd[r];
	__syncthreads();
	for (int c0 = ((N - 1) / NB) * NB; c0 >= 0; c0 -= NB) {
		const int nb = min(NB, N - c0);
		{ const int r = tid >> 5, k = tid & 31; L[r][k] = r < nb && k < r ? S[(size_t)(c0 + r) * N + c0 + k] : 0.0; }
		__syncthreads();
		for (int k = nb - 1; k > 0; --k) {
			if (tid < k) y[c0 + tid] -= L[k][tid] * y[c0 + k];
			__syncthreads();
		}
		for (int r = tid; r < c0; r += 1024) {
			double s = y[r];
			for (int k = nb - 1; k >= 0; --k) s -= S[(size_t)(c0 + k) * N + r] * y[c0 + k];
			y[r] = s;
		}
		__syncthreads();
	}
	for (int r = tid; r < N; r += 1024) d.x[r] = y[r];
}

// the trial estimates: Sim3(x_f) * estimate for a free vertex (simpleVertexSim3Expmap::oplusImpl; _fix_scale is false), the estimate for a fixed one
__global__ void k_eg_apply(EgDev d) {
	const int v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= d.nKfs) return;
	const int f = d.fidx[v];
	Sim3g S = sim3_load(d.est + 8 * (size_t)v);
	if (f >= 0) {
		double u[7];
		for (int k = 0; k < 7; ++k) u[k] = d.x[7 * f + k];
		S = sim3_mul(sim3_exp(u), S);
	}
	sim3_store(S, d.estT + 8 * (size_t)v);
}

// OptimizationAlgorithmLevenberg::solve behind the trial's evaluation (optimization_algorithm_levenberg.cpp:123-163) and — when the trial loop ends — its
// return value and the terminate action (sparse_optimizer_terminate_action.cpp:24-57) on the errors the edges hold, which are the last trial's
__global__ void k_eg_decide(EgDev d, int it) {
	if (blockIdx.x || threadIdx.x) return;
	EgCtl& c = *d.ctl;
	LmState& lm = c.lm;
	const double raw = c.sumChi;
	lm.postChi = raw;   // accepted or not: the action reads the errors the edges hold, and nothing evaluates them again behind a rejected trial
	c.accepted = lm_trial(lm, raw, c.solveOk != 0, c.sumScale) ? 1 : 0;   // computeScale: k_eg_reduce summed all of it
	EgRecord r{};
	r.more = lm_more(lm);   // no stop-flag term: the run ends behind the iteration whose action sets the flag
	r.resultOk = 1; r.why = STOP_ITERATIONS;
	if (!r.more) {
		if (const int end = lm_iter_end(lm)) { r.resultOk = 0; r.why = end; }
		if (it < 15) { if (lm_gain_stop(lm, it)) { r.stopNow = 1; if (r.resultOk) r.why = STOP_GAIN; } }
		else { r.stopNow = 1; if (r.resultOk) r.why = STOP_CAP; }   // iteration >= _maxIterations: stop without a test
	}
	r.qmax = lm.qmax; r.nonfinite = c.nonfinite; r.nEdgesOk = c.nEdgesOk; r.accepted = c.accepted;
	r.lambda = lm.lambda; r.chi2 = lm.currentChi;   // the chi2 of the estimate, not the action's last
	*d.rec = r;
}

__global__ void k_eg_accept(EgDev d) {
	if (!d.ctl->accepted) return;
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t < 8 * d.nKfs) d.est[t] = d.estT[t];
}

// ---------------------------------------------------------------------------------------------- the outputs
__global__ void k_eg_writeback(EgDev d) {
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t < d.nKfs) {
		const Sim3g S = sim3_load(d.est + 8 * (size_t)t);
		sim3_store(S, d.ScwOut + 8 * (size_t)t);
		double R[9], M[16], inv[16];
		quat_to_mat(S.q, R);
		for (int i = 0; i < 3; ++i) {
			for (int k = 0; k < 3; ++k) M[4 * i + k] = R[3 * i + k];
			M[4 * i + 3] = S.t[i] / S.s;
		}
		M[12] = M[13] = M[14] = 0.0; M[15] = 1.0;
		inv_mat(M, inv);
		for (int k = 0; k < 16; ++k) d.poseOut[16 * (size_t)t + k] = inv[k];
		if (d.kfT) for (int k = 0; k < 3; ++k) d.kfT[3 * (size_t)t + k] = inv[4 * k + 3];
	}
	if (t < d.nPoints) {
		const int r = d.ptRef[t];
		if (r >= 0 && r < d.nKfs) {   // corrected_Swr.map(Srw.map(X)), :504-510
			const double X[3] = {d.posIO[3 * (size_t)t], d.posIO[3 * (size_t)t + 1], d.posIO[3 * (size_t)t + 2]};
			double a[3], b[3];
			sim3_map(sim3_load(d.Scw + 8 * (size_t)r), X, a);
			sim3_map(sim3_inverse(sim3_load(d.est + 8 * (size_t)r)), a, b);
			for (int k = 0; k < 3; ++k) d.posIO[3 * (size_t)t + k] = b[k];
		}
	}
}

}  // namespace

// ---------------------------------------------------------------------------------------------- cOptimizer::OptimizeEssentialGraph
int mcs_optimize_essential_graph(mcs_ctx* c, int n_kfs, const double* Scw, const double* Snc, const uint8_t* has_nc, const uint8_t* kf_fixed, int n_edges,
                                 const int32_t* edge_i, const int32_t* edge_j, const uint8_t* edge_kind, int n_points, double* pos, const int32_t* pt_ref,
                                 mcs_mem_kind kind, double* Scw_out, double* pose, double* kf_t, mcs_eg_diag* diag) {
	const EgCall q{n_kfs, Scw, Snc, has_nc, kf_fixed, n_edges, edge_i, edge_j, edge_kind, n_points, pos, pt_ref, kind, Scw_out, pose, kf_t, diag};
	if (int r = guard_eg(c, q, c && c->asyncSearch)) return r;
	const bool host = kind == MCS_MEM_HOST;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	// who is free: the one thing the host must know before anything runs (the size of the system)
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
	if (int r = guard_eg_free(fixedH.data(), n_kfs, &nFree)) return r;
	if (host)
		if (int r = guard_eg_content(q)) return r;
	mcs_eg_diag dg{};
	dg.stop = STOP_NOT_RUN;
	dg.n_free = nFree;
	auto leave = [&](int status) { dg.status = status; if (diag) *diag = dg; return MCS_OK; };
	if (nFree == 0) return leave(MCS_EG_NO_FREE_VERTEX);
	if (n_edges == 0) return leave(MCS_EG_FAILED);
	if (!c->lbaRec) HIPCHK(hipHostMalloc(&c->lbaRec, 64, hipHostMallocDefault));   // the optimisers' shared 64-byte record: one call runs at a time
	volatile EgRecord* rec = (volatile EgRecord*)c->lbaRec;

	std::vector<int> fidx((size_t)n_kfs, -1), freeKf;
	for (int k = 0; k < n_kfs; ++k) if (!fixedH[k]) { fidx[k] = (int)freeKf.size(); freeKf.push_back(k); }
	const size_t K = n_kfs, P = n_points, E = n_edges, F = nFree, N = 7 * F;
	EgDev d{};
	d.nKfs = n_kfs; d.nEdges = n_edges; d.nPoints = n_points; d.nFree = nFree; d.N = (int)N;
	d.rec = (EgRecord*)device_view(c->lbaRec);
	if (!d.rec) return fail(MCS_ERR_HIP, "the control record is not visible from the device");
	Staging st(c, host);
	st.in(&d.Scw, Scw, K * 64); st.in(&d.Snc, Snc, K * 64); st.in(&d.hasNc, has_nc, K);   // kf_fixed reaches the device as fidx / freeKf
	st.in(&d.edgeI, edge_i, E * 4); st.in(&d.edgeJ, edge_j, E * 4); st.in(&d.edgeKind, edge_kind, E);
	st.inout(&d.posIO, pos, P * 24); st.in(&d.ptRef, pt_ref, P * 4);
	st.inout(&d.ScwOut, Scw_out, K * 64); st.inout(&d.poseOut, pose, K * 128);   // in/out: a status that writes nothing leaves them as they came in
	if (kf_t) st.inout(&d.kfT, kf_t, K * 24);
	st.upload(&d.fidx, fidx.data(), K * 4); st.upload(&d.freeKf, freeKf.data(), F * 4);
	st.scratch(&d.est, K * 64); st.scratch(&d.estT, K * 64); st.scratch(&d.V, K * 15 * 64); st.scratch(&d.Vinv, K * 15 * 64);
	st.scratch(&d.ok, E); st.scratch(&d.meas, E * 64); st.scratch(&d.edge, E * kEdgeDoubles * 8); st.scratch(&d.eChi, E * 8);
	st.scratch(&d.vCount, F * 4); st.scratch(&d.vOff, (F + 1) * 4); st.scratch(&d.vList, 2 * E * 4);
	st.scratch(&d.S, N * N * 8); st.scratch(&d.dd, N * 8); st.scratch(&d.b, N * 8); st.scratch(&d.x, N * 8);
	st.scratch(&d.ctl, sizeof(EgCtl));
	if (int r = st.commit()) return r;

	int status = MCS_EG_OK;
	auto sync = [&]() -> int { HIPCHK(hipStreamSynchronize(s)); return MCS_OK; };
	auto run = [&]() -> int {
		c->tic("optimize_essential_graph");
		HIPCHK(hipMemsetAsync(d.ctl, 0, sizeof(EgCtl), s));
		HIPCHK(hipMemcpyAsync(d.est, d.Scw, K * 64, hipMemcpyDeviceToDevice, s));
		HIPCHK(hipMemsetAsync(d.x, 0, N * 8, s));   // buildStructure -> Solver::resize: zeros; a failed solve leaves the last x
		hipLaunchKernelGGL(k_eg_prepare, blocks(E, 128), dim3(128), 0, s, d);
		hipLaunchKernelGGL(k_eg_lists<false>, dim3(nFree), dim3(256), 0, s, d);
		hipLaunchKernelGGL(k_eg_offsets, dim3(1), dim3(64), 0, s, d);
		hipLaunchKernelGGL(k_eg_lists<true>, dim3(nFree), dim3(256), 0, s, d);
		if (int r = sync()) return r;
		dg.n_edges = rec->nEdgesOk;
		if (dg.n_edges == 0) { status = MCS_EG_FAILED; return MCS_OK; }   // optimize() returns Fail: no write-back
		int it = 0, why = STOP_ITERATIONS;
		bool resultOk = true, stop = false;
		while (it < 20 && !stop && resultOk) {
			// ---- OptimizationAlgorithmLevenberg::solve(it): computeActiveErrors, buildSystem
			hipLaunchKernelGGL(k_eg_vertices, blocks(K * 15, 128), dim3(128), 0, s, d, d.est, 15);
			hipLaunchKernelGGL(k_eg_linearise, blocks(E, 2), dim3(64), 0, s, d);
			hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(1024), 0, s, d, 0);
			hipLaunchKernelGGL(k_eg_iter_begin, dim3(1), dim3(64), 0, s, d, it);
			while (true) {
				c->tic("eg_trial"); c->tic("eg_solve");
				HIPCHK(hipMemsetAsync(d.S, 0, N * N * 8, s));
				hipLaunchKernelGGL(k_eg_assemble, dim3(nFree), dim3(64), 0, s, d);
				for (size_t c0 = 0; c0 < N; c0 += NB) {
					const int nb = (int)std::min<size_t>(NB, N - c0);
					hipLaunchKernelGGL(k_eg_factor, dim3(1), dim3(1024), 0, s, d, (int)c0, nb);
					const size_t below = N - c0 - nb;
					if (!below) break;
					const unsigned tiles = (unsigned)((below + 63) / 64);
					hipLaunchKernelGGL(k_eg_panel, dim3(tiles), dim3(64), 0, s, d, (int)c0);
					hipLaunchKernelGGL(k_eg_trail, dim3(tiles, tiles), dim3(256), 0, s, d, (int)c0);
				}
				hipLaunchKernelGGL(k_eg_subst, dim3(1), dim3(1024), 0, s, d);
				c->toc("eg_solve");
				hipLaunchKernelGGL(k_eg_apply, blocks(K, 128), dim3(128), 0, s, d);
				hipLaunchKernelGGL(k_eg_vertices, blocks(K, 128), dim3(128), 0, s, d, d.estT, 1);
				hipLaunchKernelGGL(k_eg_residuals, blocks(E, 128), dim3(128), 0, s, d);
				hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(1024), 0, s, d, 1);
				hipLaunchKernelGGL(k_eg_decide, dim3(1), dim3(64), 0, s, d, it);
				hipLaunchKernelGGL(k_eg_accept, blocks(8 * K, 256), dim3(256), 0, s, d);
				c->toc("eg_trial");
				if (int r = sync()) return r;   // the one wait of the trial
				if (it == 0 && rec->nonfinite) { status = MCS_EG_NONFINITE; return MCS_OK; }
				if (!rec->more) break;
			}
			dg.trials[it] = rec->qmax;
			if (!rec->resultOk) { resultOk = false; why = rec->why; }
			if (rec->stopNow) { stop = true; if (resultOk) why = rec->why; }
			dg.lambda = rec->lambda; dg.chi2 = rec->chi2;
			++it;
		}
		dg.iters = it; dg.stop = why;
		hipLaunchKernelGGL(k_eg_writeback, blocks(std::max(K, P), 256), dim3(256), 0, s, d);
		return MCS_OK;
	};
	int rc = run();
	c->toc("optimize_essential_graph");
	if (rc == MCS_OK && hipGetLastError() != hipSuccess) rc = fail(MCS_ERR_HIP, "essential graph: a launch failed");
	c->lastResultStream = s;
	rc = st.finish(rc);   // a status that writes nothing leaves the in/out pieces as they were uploaded
	if (rc != MCS_OK) return rc;
	return leave(status);
}
