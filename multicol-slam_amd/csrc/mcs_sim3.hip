// mcs_sim3.hip — cSim3Solver (src/cSim3Solver.cpp, include/cSim3Solver.h) for a batch of loop candidates: the RANSAC of
// cLoopClosing::ComputeSim3 (src/cLoopClosing.cpp:300-330).
//   k_sim3_setup    one thread per correspondence: the constructor's arithmetic (:100-131): X3Dc = Hom2R(M_t^-1) Xw + Hom2T(M_t^-1), the
//                   projection into its own keyframe (WorldToCamHom_fast, src/cam_system_omni.cpp:114-133), the size_t thresholds 9.210 sigma^2;
//                   threads below nr_cams also form invMat(M_c(c)) of the local rig, once per camera
//   k_sim3_hyp      one thread per (solver, iteration): the three draws with the reference's index handling (:202-222), computeT (:286-371,
//                   Horn 1987 with OpenCV's Jacobi eigen solver and Rodrigues), mT12i and mT21i
//   k_sim3_score    one wave per (solver, iteration): CheckInliers (:374-415), lanes walk the correspondences, __ballot gives 64 inlier bits
//   k_sim3_scan     one thread per solver: the rules of one iterate() call (:167-254) over the counts, in iteration order; the solver state
//                   (mnIterations, mnBestInliers, mBest*) stays on the device
//   k_sim3_inliers  one thread per correspondence: vbInliers[mvnIndices1[i]] of a solver whose call succeeded
// Only the iterations a call can reach are evaluated: [mnIterations, min(mnIterations + n, mRansacMaxIts)).  A hypothesis is a function of
// (seed or caller draws, solver, iteration) alone, so the outputs do not depend on how the iterations are split into calls.
// FP64 throughout, no contraction (-ffp-contract=off): every product and sum is the reference's, in the reference's order.
#include "mcs_host.h"
#include "mcs_geom.h"
#include <algorithm>
#include <cfloat>
#include <climits>

namespace mcs {

constexpr int kSim3MaxCams = 32;
constexpr int kHypDoubles = 45;   // T12[16] T21[16] R[9] t[3] s

struct Sim3Corr {           // one correspondence kept by the constructor
	double X1c[3], X2c[3];  // mvX3Dc1 / mvX3Dc2 (rig frame of each keyframe)
	double p1[2], p2[2];    // mvP1im1 / mvP2im2
	double e1, e2;          // mvnMaxError1 / 2: the size_t values as doubles
	int c1, c2;             // camIdx1 / camIdx2
};

struct Sim3Solver {         // per solver; the RANSAC parameters change only through mcs_sim3_set_ransac_parameters
	int N, corrOff, mN1, vbOff;
	int minInliers, maxIts;      // mRansacMinInliers, mRansacMaxIts (after SetRansacParameters; 0 when N < minInliers)
	int drawOff, nDraws;         // caller draws: offset into the draw array and iterations covered; drawOff < 0: generated
	long long maskWords;         // words of one inlier mask (ceil(N / 64))
};

struct Sim3State {          // the RANSAC state between calls
	int mnIterations, mnBestInliers;
	double bestT12[16], bestR[9], bestt[3], bestS;
};

struct Sim3Slot { int solver, iter; long long maskOff; };   // one hypothesis of a call

struct Sim3Out { int success, noMore, nInliers, mnIterations; double T12[16]; long long succMask; };

struct Sim3SetupArgs {
	int nc, nrCams;
	const double* Mc;           // [nrCams][16] M_c of the local rig
	double* McInv;              // [nrCams][16] invMat(M_c)
	const int* corrSolver;      // [nc]
	const double* Mtinv;        // [ns][2][16]
	const double* MtMcInv;      // [ns][2][nrCams][16]
	const OcamDev* cams;        // [nrCams]
	const double* Xw;           // [nc][2][3]
	const int* cam;             // [nc][2]
	const double* sigma2;       // [nc][2]
	Sim3Corr* corr;
};

__global__ __launch_bounds__(64) void k_sim3_setup(Sim3SetupArgs a) {
	const int g = blockIdx.x * 64 + threadIdx.x;
	if (g < a.nrCams) inv_mat(a.Mc + 16 * (size_t)g, a.McInv + 16 * (size_t)g);
	if (g >= a.nc) return;
	const int s = a.corrSolver[g];
	Sim3Corr c;
#pragma unroll
	for (int side = 0; side < 2; ++side) {
		const double* X = a.Xw + 6 * (size_t)g + 3 * side;
		const double* hom = a.Mtinv + 32 * (size_t)s + 16 * side;
		const int cam = a.cam[2 * (size_t)g + side];
		double* Xc = side ? c.X2c : c.X1c;
		matx44_point<3>(hom, X, Xc);   // Hom2R(hom) * X + Hom2T(hom): the same sums, the last term being hom(i,3) * 1.0
		double* p = side ? c.p2 : c.p1;
		(void)world_to_cam_hom_fast(a.MtMcInv + ((size_t)s * 2 + side) * a.nrCams * 16 + 16 * (size_t)cam, a.cams[cam], X[0], X[1], X[2], p[0], p[1]);
		const double e = 9.210 * a.sigma2[2 * (size_t)g + side];   // mvnMaxError is a std::vector<size_t>: the product is truncated
		const double et = (double)(unsigned long long)e;
		if (side) { c.e2 = et; c.c2 = cam; } else { c.e1 = et; c.c1 = cam; }
	}
	a.corr[g] = c;
}

// ---------------------------------------------------------------------------------------------- the draws
// output number ctr + 1 of the splitmix64 stream at `seed`, ctr = (solver << 32) | (3 k + j), mapped to [0, N) by (hi32 * N) >> 32
__host__ __device__ __forceinline__ int sim3_draw(unsigned long long seed, int solver, int k, int j, int N) {
	unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (((((unsigned long long)(unsigned)solver) << 32) | (unsigned long long)(3u * (unsigned)k + (unsigned)j)) + 1ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	z ^= z >> 31;
	return (int)(((z >> 32) * (unsigned long long)(unsigned)N) >> 32);
}

// ---------------------------------------------------------------------------------------------- computeT
// OpenCV's hypot of the Jacobi solver (modules/core/src/lapack.cpp)
__device__ __forceinline__ double cv_hypot(double a, double b) {
	a = fabs(a); b = fabs(b);
	if (a > b) { b /= a; return a * sqrt(1 + b * b); }
	if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
	return 0;
}

// cv::eigen of a symmetric 4x4 (JacobiImpl_, modules/core/src/lapack.cpp): W descending, V rows = eigenvectors
__device__ void jacobi4(double* A, double* W, double* V) {
	const int n = 4;
	const double eps = DBL_EPSILON;
	int indR[4], indC[4];
	for (int i = 0; i < n; ++i) {
		for (int j = 0; j < n; ++j) V[i * n + j] = 0.0;
		V[i * n + i] = 1.0;
	}
	double mv;
	int m, i, k;
	indR[n - 1] = 0; indC[0] = 0;
	for (k = 0; k < n; k++) {
		W[k] = A[(n + 1) * k];
		if (k < n - 1) {
			for (m = k + 1, mv = fabs(A[n * k + m]), i = k + 2; i < n; i++) {
				const double val = fabs(A[n * k + i]);
				if (mv < val) mv = val, m = i;
			}
			indR[k] = m;
		}
		if (k > 0) {
			for (m = 0, mv = fabs(A[k]), i = 1; i < k; i++) {
				const double val = fabs(A[n * i + k]);
				if (mv < val) mv = val, m = i;
			}
			indC[k] = m;
		}
	}
	for (int iters = 0; iters < n * n * 30; iters++) {
		for (k = 0, mv = fabs(A[indR[0]]), i = 1; i < n - 1; i++) {
			const double val = fabs(A[n * i + indR[i]]);
			if (mv < val) mv = val, k = i;
		}
		int l = indR[k];
		for (i = 1; i < n; i++) {
			const double val = fabs(A[n * indC[i] + i]);
			if (mv < val) mv = val, k = indC[i], l = i;
		}
		const double p = A[n * k + l];
		if (fabs(p) <= eps) break;
		const double y = (W[l] - W[k]) * 0.5;
		double t = fabs(y) + cv_hypot(p, y);
		double s = cv_hypot(p, t);
		const double c = t / s;
		s = p / s; t = (p / t) * p;
		if (y < 0) s = -s, t = -t;
		A[n * k + l] = 0;
		W[k] -= t;
		W[l] += t;
		double a0, b0;
#define MCS_ROT(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
		for (i = 0; i < k; i++) MCS_ROT(A[n * i + k], A[n * i + l]);
		for (i = k + 1; i < l; i++) MCS_ROT(A[n * k + i], A[n * i + l]);
		for (i = l + 1; i < n; i++) MCS_ROT(A[n * k + i], A[n * l + i]);
		for (i = 0; i < n; i++) MCS_ROT(V[n * k + i], V[n * l + i]);
#undef MCS_ROT
		for (int j = 0; j < 2; j++) {
			const int idx = j == 0 ? k : l;
			if (idx < n - 1) {
				for (m = idx + 1, mv = fabs(A[n * idx + m]), i = idx + 2; i < n; i++) {
					const double val = fabs(A[n * idx + i]);
					if (mv < val) mv = val, m = i;
				}
				indR[idx] = m;
			}
			if (idx > 0) {
				for (m = 0, mv = fabs(A[idx]), i = 1; i < idx; i++) {
					const double val = fabs(A[n * i + idx]);
					if (mv < val) mv = val, m = i;
				}
				indC[idx] = m;
			}
		}
	}
	for (k = 0; k < n - 1; k++) {   // selection sort, descending; eigenvector rows move with their values
		m = k;
		for (i = k + 1; i < n; i++)
			if (W[m] < W[i]) m = i;
		if (k != m) {
			double tmp = W[m]; W[m] = W[k]; W[k] = tmp;
			for (i = 0; i < n; i++) { tmp = V[n * m + i]; V[n * m + i] = V[n * k + i]; V[n * k + i] = tmp; }
		}
	}
}

// centroid (:264-284): C = the sum of the columns, C /= 3.0 as OpenCV's Vec operator/= (a multiplication by 1. / alpha)
__device__ __forceinline__ void centroid(const double* P, double* Pr, double* C) {
	for (int r = 0; r < 3; ++r) {
		double acc = 0.0;
		for (int i = 0; i < 3; ++i) acc += P[3 * r + i];
		C[r] = acc;
	}
	const double ia = 1. / 3.0;
	for (int r = 0; r < 3; ++r) C[r] = C[r] * ia;
	for (int r = 0; r < 3; ++r)
		for (int i = 0; i < 3; ++i) Pr[3 * r + i] = P[3 * r + i] - C[r];
}

// computeT (:286-371); P1, P2 row-major 3x3 with one point per column; out = T12[16] T21[16] R[9] t[3] s
__device__ void compute_t(const double* P1, const double* P2, double* out) {
	double Pr1[9], Pr2[9], O1[3], O2[3];
	centroid(P1, Pr1, O1);
	centroid(P2, Pr2, O2);
	double M[9];   // Pr2 * Pr1.t()
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			double acc = 0;
			for (int k = 0; k < 3; ++k) acc += Pr2[3 * i + k] * Pr1[3 * j + k];
			M[3 * i + j] = acc;
		}
	const double N11 = M[0] + M[4] + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3], N22 = M[0] - M[4] - M[8], N23 = M[1] + M[3],
	             N24 = M[6] + M[2], N33 = -M[0] + M[4] - M[8], N34 = M[5] + M[7], N44 = -M[0] - M[4] + M[8];
	double A[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
	double W[4], V[16];
	jacobi4(A, W, V);
	double vec[3] = {V[1], V[2], V[3]};
	const double nv = sqrt(((0 + vec[0] * vec[0]) + vec[1] * vec[1]) + vec[2] * vec[2]);   // cv::norm
	const double ang = atan2(nv, V[0]);
	const double f = (2 * ang) * (1. / nv);   // 2 * ang * vec / norm(vec): one MatExpr scale factor
	for (int i = 0; i < 3; ++i) vec[i] = vec[i] * f;
	double R[9];   // cv::Rodrigues
	{
		double rx = vec[0], ry = vec[1], rz = vec[2];
		const double theta = sqrt(rx * rx + ry * ry + rz * rz);
		if (theta < DBL_EPSILON) {
			for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
		} else {
			const double c = cos(theta), s = sin(theta), c1 = 1. - c;
			const double itheta = theta ? 1. / theta : 0.;
			rx *= itheta; ry *= itheta; rz *= itheta;
			const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
			const double rx_[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
			const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
			for (int k = 0; k < 9; ++k) R[k] = c * I[k] + c1 * rrt[k] + s * rx_[k];
		}
	}
	double P3[9];   // mR12i * Pr2
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			double acc = 0;
			for (int k = 0; k < 3; ++k) acc += R[3 * i + k] * Pr2[3 * k + j];
			P3[3 * i + j] = acc;
		}
	double nom = 0;   // Pr1.dot(P3), row-major
	for (int k = 0; k < 9; ++k) nom += Pr1[k] * P3[k];
	double den = 0;   // cv::pow(P3, 2) summed row by row
	for (int k = 0; k < 9; ++k) den += P3[k] * P3[k];
	const double s = nom / den;
	double sR[9], t[3];
	for (int k = 0; k < 9; ++k) sR[k] = R[k] * s;   // ms12i * mR12i
	for (int i = 0; i < 3; ++i) {   // O1 - (ms12i * mR12i) * O2
		double acc = 0;
		for (int k = 0; k < 3; ++k) acc += sR[3 * i + k] * O2[k];
		t[i] = O1[i] - acc;
	}
	const double is = 1.0 / s;
	double sRinv[9], tinv[3];
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) sRinv[3 * i + j] = R[3 * j + i] * is;
	for (int i = 0; i < 3; ++i) {   // -sRinv * mt12i
		double acc = 0;
		for (int k = 0; k < 3; ++k) acc += -sRinv[3 * i + k] * t[k];
		tinv[i] = acc;
	}
	double* T12 = out;
	double* T21 = out + 16;
	for (int i = 0; i < 3; ++i) {   // Rt2Hom
		for (int j = 0; j < 3; ++j) { T12[4 * i + j] = sR[3 * i + j]; T21[4 * i + j] = sRinv[3 * i + j]; }
		T12[4 * i + 3] = t[i]; T21[4 * i + 3] = tinv[i];
	}
	T12[12] = T12[13] = T12[14] = 0.0; T12[15] = 1.0;
	T21[12] = T21[13] = T21[14] = 0.0; T21[15] = 1.0;
	for (int k = 0; k < 9; ++k) out[32 + k] = R[k];
	for (int k = 0; k < 3; ++k) out[41 + k] = t[k];
	out[44] = s;
}

struct Sim3HypArgs {
	int nSlots;
	const Sim3Slot* slots; const Sim3Solver* solvers; const Sim3Corr* corr;
	const int* draws; unsigned long long seed;
	double* hyp; int* picks;
};

__global__ __launch_bounds__(64) void k_sim3_hyp(Sim3HypArgs a) {
	const int h = blockIdx.x * 64 + threadIdx.x;
	if (h >= a.nSlots) return;
	const Sim3Slot sl = a.slots[h];
	const Sim3Solver S = a.solvers[sl.solver];
	const int N = S.N;
	// vAvailableIndices = mvAllIndices as a fixed array of N entries: pop_back leaves the stale value in place, so only this iteration's writes
	// differ from the identity; the distribution keeps [0, N - 1] and the write goes to slot idx, not randi (:202-221)
	int wpos[3], wval[3], nw = 0, size = N;
	auto at = [&](int x) { int v = x; for (int q = 0; q < nw; ++q) if (wpos[q] == x) v = wval[q]; return v; };
	double P1[9], P2[9];
	for (int j = 0; j < 3; ++j) {
		const int randi = S.drawOff >= 0 ? a.draws[S.drawOff + 3 * sl.iter + j] : sim3_draw(a.seed, sl.solver, sl.iter, j, N);
		const int idx = at(randi);
		const Sim3Corr& c = a.corr[S.corrOff + idx];
		for (int r = 0; r < 3; ++r) { P1[3 * r + j] = c.X1c[r]; P2[3 * r + j] = c.X2c[r]; }
		a.picks[3 * (size_t)h + j] = idx;
		const int back = at(size - 1);
		wpos[nw] = idx; wval[nw] = back; ++nw;
		--size;
	}
	compute_t(P1, P2, a.hyp + (size_t)h * kHypDoubles);
}

struct Sim3ScoreArgs {
	int nSlots, nrCams;
	const Sim3Slot* slots; const Sim3Solver* solvers; const Sim3Corr* corr;
	const double* McInv; const OcamDev* cams; const double* hyp;
	unsigned long long* masks; int* counts;
};

__global__ __launch_bounds__(256) void k_sim3_score(Sim3ScoreArgs a) {
	__shared__ double sM[kSim3MaxCams * 12];   // rows 0..2 of invMat(M_c) per camera
	__shared__ OcamDev sCam[kSim3MaxCams];
	for (int i = threadIdx.x; i < a.nrCams * 12; i += 256) sM[i] = a.McInv[16 * (i / 12) + i % 12];
	for (int i = threadIdx.x; i < a.nrCams; i += 256) sCam[i] = a.cams[i];
	__syncthreads();
	const int h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (h >= a.nSlots) return;
	const Sim3Slot sl = a.slots[h];
	const Sim3Solver S = a.solvers[sl.solver];
	const double* T12 = a.hyp + (size_t)h * kHypDoubles;
	const double* T21 = T12 + 16;
	double A[16], B[16];
	for (int k = 0; k < 16; ++k) { A[k] = T12[k]; B[k] = T21[k]; }
	const Sim3Corr* corr = a.corr + S.corrOff;
	unsigned long long* mask = a.masks + sl.maskOff;
	int count = 0;
	for (int base = 0; base < S.N; base += 64) {
		const int i = base + lane;
		bool in = false;
		if (i < S.N) {
			const Sim3Corr c = corr[i];
			const double x2[4] = {c.X2c[0], c.X2c[1], c.X2c[2], 1.0}, x1[4] = {c.X1c[0], c.X1c[1], c.X1c[2], 1.0};
			double p21[4], p12[4], r1[3], r2[3];
			matx44_vec4<4>(A, x2, p21);   // mT12i * (X3Dc2, 1)
			matx44_vec4<4>(B, x1, p12);   // mT21i * (X3Dc1, 1)
			matx44_vec4<3>(sM + 12 * c.c1, p21, r1);   // invMat(M_c(camIdx1)) * pt2_in_1
			matx44_vec4<3>(sM + 12 * c.c2, p12, r2);   // invMat(M_c(camIdx2)) * pt1_in_2
			double u1, v1, u2, v2;
			omni_world_to_img(sCam[c.c1], r1[0], r1[1], r1[2], u1, v1);
			omni_world_to_img(sCam[c.c2], r2[0], r2[1], r2[2], u2, v2);
			const double d10 = c.p1[0] - u1, d11 = c.p1[1] - v1;   // mvP1im1[i] - vP2im1
			const double d20 = u2 - c.p2[0], d21 = v2 - c.p2[1];   // vP1im2 - mvP2im2[i]
			const double err1 = d10 * d10 + d11 * d11, err2 = d20 * d20 + d21 * d21;
			in = err1 < c.e1 && err2 < c.e2;
		}
		const unsigned long long bits = __ballot(in);
		if (lane == 0) mask[base >> 6] = bits;
		count += __popcll(bits);
	}
	if (lane == 0) a.counts[h] = count;
}

struct Sim3ScanArgs {
	int ns;
	const int* nIt;           // [ns] iterations asked for (<= 0: the solver is left alone)
	const int* slotOff;       // [ns + 1]
	const Sim3Slot* slots; const Sim3Solver* solvers; const double* hyp; const int* counts;
	Sim3State* state; Sim3Out* out;
};

__global__ __launch_bounds__(64) void k_sim3_scan(Sim3ScanArgs a) {
	const int s = blockIdx.x * 64 + threadIdx.x;
	if (s >= a.ns) return;
	Sim3Out o;
	o.success = 0; o.noMore = 0; o.nInliers = 0; o.succMask = -1;
	for (int k = 0; k < 16; ++k) o.T12[k] = 0.0;
	const Sim3Solver S = a.solvers[s];
	Sim3State& st = a.state[s];
	int mnIt = st.mnIterations;
	if (a.nIt[s] > 0) {
		if (S.N < S.minInliers) {
			o.noMore = 1;
		} else {
			int bestInl = st.mnBestInliers, bestSlot = -1;   // the state is written once, after the walk
			for (int h = a.slotOff[s]; h < a.slotOff[s + 1]; ++h) {
				++mnIt;
				const int cnt = a.counts[h];
				if (cnt >= bestInl) {   // also 0 >= 0
					bestInl = cnt;
					bestSlot = h;
					if (cnt > S.minInliers) {   // returns at once: mnIterations stops here and bNoMore stays false
						o.success = 1; o.nInliers = cnt; o.succMask = a.slots[h].maskOff;
						break;
					}
				}
			}
			if (bestSlot >= 0) {
				const double* H = a.hyp + (size_t)bestSlot * kHypDoubles;
				st.mnBestInliers = bestInl;
				for (int k = 0; k < 16; ++k) st.bestT12[k] = H[k];
				for (int k = 0; k < 9; ++k) st.bestR[k] = H[32 + k];
				for (int k = 0; k < 3; ++k) st.bestt[k] = H[41 + k];
				st.bestS = H[44];
				if (o.success)
					for (int k = 0; k < 16; ++k) o.T12[k] = H[k];
			}
			st.mnIterations = mnIt;
			if (!o.success && mnIt >= S.maxIts) o.noMore = 1;
		}
	}
	o.mnIterations = mnIt;
	a.out[s] = o;
}

__global__ __launch_bounds__(256) void k_sim3_inliers(int nc, const int* corrSolver, const int* index1, const Sim3Solver* solvers, const Sim3Out* out,
                                                      const unsigned long long* masks, uint8_t* vb) {
	const int g = blockIdx.x * 256 + threadIdx.x;
	if (g >= nc) return;
	const int s = corrSolver[g];
	const long long m = out[s].succMask;
	if (m < 0) return;
	const int i = g - solvers[s].corrOff;
	if ((masks[m + (i >> 6)] >> (i & 63)) & 1ull) vb[solvers[s].vbOff + index1[g]] = 1;
}

}  // namespace mcs

using namespace mcs;

struct mcs_sim3 {
	mcs_ctx* ctx = nullptr;
	int ns = 0, nc = 0, nrCams = 0, sumN1 = 0;
	unsigned long long seed = 0;
	std::vector<Sim3Solver> solvers;   // host copy of the per-solver constants
	std::vector<int> mnIt;             // host copy of mnIterations (read back by every call)
	uint8_t* dev = nullptr;            // constants and state, one allocation
	OcamDev* dCams = nullptr; double* dMcInv = nullptr; Sim3Solver* dSolvers = nullptr; Sim3Corr* dCorr = nullptr; int* dCorrSolver = nullptr;
	int* dIndex1 = nullptr; int* dDraws = nullptr; Sim3State* dState = nullptr;
	Sim3Out* hOut = nullptr; size_t hOutCap = 0;   // page-locked read-back
};

namespace {

// SetRansacParameters (:139-165): the iteration count, with the double -> int conversion of x86-64 (cvttsd2si: INT_MIN when out of range or NaN)
int ransac_max_its(double probability, int minInliers, int maxIterations, int N) {
	const double epsilon = (double)minInliers / N;
	int nIterations;
	if (minInliers == N) nIterations = 1;
	else {
		const double d = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
		nIterations = (d >= -2147483648.0 && d < 2147483648.0) ? (int)d : INT_MIN;
	}
	return std::max(1, std::min(nIterations, maxIterations));
}

// the slots of solver s's iterations [first, first + count), mask offsets continuing from `words`
void add_slots(const mcs_sim3* b, int s, int first, int count, std::vector<Sim3Slot>& slots, long long& words) {
	for (int k = 0; k < count; ++k) {
		slots.push_back(Sim3Slot{s, first + k, words});
		words += b->solvers[s].maskWords;
	}
}

// hypotheses and scores of `slots`: declared on the call's staging (the destinations are optional), launched after its commit
struct Eval { const Sim3Slot* slots; double* hyp; int* picks; unsigned long long* masks; int* counts; };
void eval_stage(Staging& st, const std::vector<Sim3Slot>& slots, long long words, Eval& ev, double* hypOut, int32_t* picksOut, unsigned long long* masksOut, int32_t* countsOut) {
	const size_t H = slots.size();
	st.upload(&ev.slots, slots.data(), H * sizeof(Sim3Slot));
	st.out(&ev.hyp, hypOut, H * kHypDoubles * 8); st.out(&ev.picks, picksOut, H * 12); st.out(&ev.masks, masksOut, (size_t)words * 8); st.out(&ev.counts, countsOut, H * 4);
}
int eval_launch(mcs_sim3* b, size_t H, const Eval& ev) {
	if (!H) return MCS_OK;
	hipStream_t st = b->ctx->stream;
	Sim3HypArgs ha{(int)H, ev.slots, b->dSolvers, b->dCorr, b->dDraws, b->seed, ev.hyp, ev.picks};
	hipLaunchKernelGGL(k_sim3_hyp, dim3((unsigned)((H + 63) / 64)), dim3(64), 0, st, ha);
	Sim3ScoreArgs sa{(int)H, b->nrCams, ev.slots, b->dSolvers, b->dCorr, b->dMcInv, b->dCams, (const double*)ev.hyp, ev.masks, ev.counts};
	hipLaunchKernelGGL(k_sim3_score, dim3((unsigned)((H + 3) / 4)), dim3(256), 0, st, sa);
	HIPCHK(hipGetLastError());
	return MCS_OK;
}

}  // namespace

int mcs_sim3_destroy(mcs_sim3* b) {
	if (!b) return MCS_OK;
	(void)hipSetDevice(b->ctx->device);
	(void)hipFree(b->dev);
	if (b->hOut) (void)hipHostFree(b->hOut);
	delete b;
	return MCS_OK;
}

int mcs_sim3_create(mcs_ctx* c, int nr_cams, const double* M_c, const mcs_ocam* cams, int n_solvers, const int32_t* mN1, const int32_t* corr_offsets,
                    const double* M_t_inv, const double* MtMc_inv, const double* probability, const int32_t* min_inliers, const int32_t* max_iterations,
                    const double* Xw, const int32_t* cam, const double* sigma2, const int32_t* index1, uint64_t seed, const int32_t* draws, mcs_sim3** out) {
	if (!c || !out) return fail(MCS_ERR_INVALID, "null argument");
	if (nr_cams < 1 || nr_cams > kSim3MaxCams) return fail(MCS_ERR_INVALID, "mcs_sim3_create: nr_cams must be in 1..32");
	if (n_solvers < 0) return fail(MCS_ERR_INVALID, "mcs_sim3_create: n_solvers must be >= 0");
	if (!M_c || !cams || (n_solvers && (!mN1 || !corr_offsets || !M_t_inv || !MtMc_inv || !probability || !min_inliers || !max_iterations)))
		return fail(MCS_ERR_INVALID, "null argument");
	const int ns = n_solvers;
	if (ns && corr_offsets[0] != 0) return fail(MCS_ERR_INVALID, "mcs_sim3_create: corr_offsets[0] must be 0");
	for (int s = 0; s < ns; ++s)
		if (corr_offsets[s + 1] < corr_offsets[s]) return fail(MCS_ERR_INVALID, "mcs_sim3_create: corr_offsets must be non-decreasing");
	const int nc = ns ? corr_offsets[ns] : 0;
	if (nc && (!Xw || !cam || !sigma2 || !index1)) return fail(MCS_ERR_INVALID, "null correspondence array");
	std::vector<OcamDev> hc(nr_cams);
	for (int i = 0; i < nr_cams; ++i)
		if (int r = ocam_to_dev(cams[i], &hc[i])) return r;
	std::vector<Sim3Solver> sv(ns);
	std::vector<int> corrSolver(nc);
	int vb = 0, drawOff = 0;
	for (int s = 0; s < ns; ++s) {
		Sim3Solver& S = sv[s];
		const std::string who = "mcs_sim3_create: solver " + std::to_string(s);
		S.N = corr_offsets[s + 1] - corr_offsets[s];
		S.corrOff = corr_offsets[s];
		S.mN1 = mN1[s];
		S.vbOff = vb;
		S.maskWords = (S.N + 63) / 64;
		if (S.mN1 < S.N) return fail(MCS_ERR_INVALID, who + ": mN1 is smaller than its number of correspondences");
		vb += S.mN1;
		for (int i = S.corrOff; i < S.corrOff + S.N; ++i) {
			corrSolver[i] = s;
			if (index1[i] < 0 || index1[i] >= S.mN1) return fail(MCS_ERR_INVALID, who + ": index1 outside [0, mN1)");
			if (cam[2 * i] < 0 || cam[2 * i] >= nr_cams || cam[2 * i + 1] < 0 || cam[2 * i + 1] >= nr_cams) return fail(MCS_ERR_INVALID, who + ": camera index out of range");
			for (int side = 0; side < 2; ++side) {   // 9.210 sigma^2 becomes a size_t (k_sim3_setup): NaN, negative and >= 2^64 have no defined conversion
				const double e = 9.210 * sigma2[2 * (size_t)i + side];
				if (!(e >= 0.0 && e < 18446744073709551616.0)) return fail(MCS_ERR_INVALID, who + ": 9.210 * sigma2 is NaN, negative or >= 2^64");
			}
		}
		S.minInliers = min_inliers[s];
		S.maxIts = 0;
		if (S.N >= S.minInliers) {
			if (S.N < 3)
				return fail(MCS_ERR_INVALID, who + " has " + std::to_string(S.N) + " correspondences and minInliers <= N: the reference is undefined there "
				                                    "(three draws from fewer than three, back() of an empty vector)");
			S.maxIts = ransac_max_its(probability[s], S.minInliers, max_iterations[s], S.N);
		}
		S.drawOff = draws ? drawOff : -1;
		S.nDraws = draws ? std::max(1, max_iterations[s]) : 0;
		if (draws) {
			if (S.N >= 3)
				for (int k = 0; k < 3 * S.nDraws; ++k)
					if (draws[drawOff + k] < 0 || draws[drawOff + k] >= S.N) return fail(MCS_ERR_INVALID, who + ": a draw is outside [0, N)");
			drawOff += 3 * S.nDraws;
		}
	}
	HIPCHK(hipSetDevice(c->device));
	mcs_sim3* b = new mcs_sim3();
	b->ctx = c; b->ns = ns; b->nc = nc; b->nrCams = nr_cams; b->seed = seed; b->sumN1 = vb;
	b->solvers = sv; b->mnIt.assign(ns, 0);
	// the object's constants and state are one allocation of its own, laid out by the staging that uploads them: the eleven arrays go up in one copy
	Staging stg(c, true);
	const double *dMc = nullptr, *dMt = nullptr, *dMtMc = nullptr, *dX = nullptr, *dSig = nullptr; const int* dCam = nullptr;
	stg.upload(&b->dCams, hc.data(), sizeof(OcamDev) * nr_cams); stg.in(&dMc, M_c, (size_t)nr_cams * 128); stg.upload(&b->dSolvers, sv.data(), sizeof(Sim3Solver) * ns);
	stg.upload(&b->dCorrSolver, corrSolver.data(), 4 * (size_t)nc); stg.in(&b->dIndex1, index1, 4 * (size_t)nc); stg.in(&b->dDraws, draws, 4 * (size_t)drawOff);
	stg.in(&dMt, M_t_inv, (size_t)ns * 256); stg.in(&dMtMc, MtMc_inv, (size_t)ns * 2 * nr_cams * 128); stg.in(&dX, Xw, (size_t)nc * 48); stg.in(&dCam, cam, (size_t)nc * 8);
	stg.in(&dSig, sigma2, (size_t)nc * 16);   // (nc == 0: the correspondence arrays may be null and stay null on the device; every kernel that reads them is bounded by nc)
	stg.scratch(&b->dMcInv, (size_t)nr_cams * 128); stg.scratch(&b->dCorr, sizeof(Sim3Corr) * nc); stg.scratch(&b->dState, sizeof(Sim3State) * ns);
	auto bail = [&](hipError_t e, const char* what) { mcs_sim3_destroy(b); return fail(MCS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); };
	hipError_t e = hipMalloc((void**)&b->dev, stg.bytes());
	if (e != hipSuccess) return bail(e, "mcs_sim3_create: allocation");
	hipStream_t st = c->stream;
	if (int r = stg.commit(b->dev)) { mcs_sim3_destroy(b); return r; }
	if (ns && (e = hipMemsetAsync(b->dState, 0, sizeof(Sim3State) * ns, st)) != hipSuccess) return bail(e, "mcs_sim3_create: state");
	Sim3SetupArgs sa{nc, nr_cams, dMc, b->dMcInv, b->dCorrSolver, dMt, dMtMc, b->dCams, dX, dCam, dSig, b->dCorr};
	hipLaunchKernelGGL(k_sim3_setup, dim3((unsigned)((std::max(nc, nr_cams) + 63) / 64)), dim3(64), 0, st, sa);
	if ((e = hipGetLastError()) != hipSuccess) return bail(e, "mcs_sim3_create: setup");
	if (int r = stg.finish(MCS_OK)) { mcs_sim3_destroy(b); return r; }
	*out = b;
	return MCS_OK;
}

int mcs_sim3_set_ransac_parameters(mcs_sim3* b, const double* probability, const int32_t* min_inliers, const int32_t* max_iterations) {
	if (!b || (b->ns && (!probability || !min_inliers || !max_iterations))) return fail(MCS_ERR_INVALID, "null argument");
	std::vector<Sim3Solver> sv = b->solvers;
	for (int s = 0; s < b->ns; ++s) {
		Sim3Solver& S = sv[s];
		const std::string who = "mcs_sim3_set_ransac_parameters: solver " + std::to_string(s);
		S.minInliers = min_inliers[s];
		S.maxIts = 0;
		if (S.N >= S.minInliers) {
			if (S.N < 3) return fail(MCS_ERR_INVALID, who + " has fewer than 3 correspondences and minInliers <= N (undefined in the reference)");
			S.maxIts = ransac_max_its(probability[s], S.minInliers, max_iterations[s], S.N);
			if (S.drawOff >= 0 && S.maxIts > S.nDraws) return fail(MCS_ERR_INVALID, who + ": the caller's draws cover fewer iterations");
		}
	}
	HIPCHK(hipSetDevice(b->ctx->device));
	hipStream_t st = b->ctx->stream;
	if (b->ns) HIPCHK(hipMemcpyAsync(b->dSolvers, sv.data(), sizeof(Sim3Solver) * b->ns, hipMemcpyHostToDevice, st));
	for (int s = 0; s < b->ns; ++s)   // mnIterations = 0; mnBestInliers and mBest* stay, as in the reference
		HIPCHK(hipMemsetAsync(&b->dState[s].mnIterations, 0, sizeof(int), st));
	HIPCHK(hipStreamSynchronize(st));
	b->solvers = sv;
	for (int s = 0; s < b->ns; ++s) b->mnIt[s] = 0;
	return MCS_OK;
}

int mcs_sim3_info(const mcs_sim3* b, int32_t* n, int32_t* max_its, int32_t* iterations) {
	if (!b) return fail(MCS_ERR_INVALID, "null argument");
	for (int s = 0; s < b->ns; ++s) {
		if (n) n[s] = b->solvers[s].N;
		if (max_its) max_its[s] = b->solvers[s].maxIts;
		if (iterations) iterations[s] = b->mnIt[s];
	}
	return MCS_OK;
}

int mcs_sim3_iterate(mcs_sim3* b, const int32_t* n_iterations, uint8_t* success, uint8_t* no_more, int32_t* n_inliers, double* T12, uint8_t* inliers) {
	if (!b || (b->ns && (!n_iterations || !success || !no_more || !n_inliers))) return fail(MCS_ERR_INVALID, "null argument");
	const int ns = b->ns;
	if (!ns) return MCS_OK;
	HIPCHK(hipSetDevice(b->ctx->device));
	hipStream_t st = b->ctx->stream;
	std::vector<Sim3Slot> slots;
	std::vector<int> slotOff(ns + 1, 0), nIt(ns);
	long long words = 0;
	for (int s = 0; s < ns; ++s) {
		const Sim3Solver& S = b->solvers[s];
		nIt[s] = n_iterations[s];
		slotOff[s] = (int)slots.size();
		if (nIt[s] > 0 && S.N >= S.minInliers) {
			const int first = b->mnIt[s];
			const int last = (int)std::min<long long>((long long)first + nIt[s], (long long)S.maxIts);
			if (last > first) add_slots(b, s, first, last - first, slots, words);
		}
	}
	slotOff[ns] = (int)slots.size();
	if (b->hOutCap < (size_t)ns) {
		if (b->hOut) (void)hipHostFree(b->hOut);
		b->hOut = nullptr; b->hOutCap = 0;
		HIPCHK(hipHostMalloc((void**)&b->hOut, sizeof(Sim3Out) * ns, hipHostMallocDefault));
		b->hOutCap = ns;
	}
	const bool wantInliers = inliers && b->sumN1;
	Staging stg(b->ctx, true);
	Eval ev{};
	eval_stage(stg, slots, words, ev, nullptr, nullptr, nullptr, nullptr);
	const int *dNIt = nullptr, *dOff = nullptr; Sim3Out* dOut = nullptr; uint8_t* dVb = nullptr;
	stg.upload(&dNIt, nIt.data(), 4 * (size_t)ns); stg.upload(&dOff, slotOff.data(), 4 * ((size_t)ns + 1));
	stg.out(&dOut, b->hOut, sizeof(Sim3Out) * ns); stg.out(&dVb, wantInliers ? inliers : nullptr, (size_t)b->sumN1);
	if (int r = stg.commit()) return r;
	if (int r = eval_launch(b, slots.size(), ev)) return r;
	Sim3ScanArgs sa{ns, dNIt, dOff, ev.slots, b->dSolvers, (const double*)ev.hyp, (const int*)ev.counts, b->dState, dOut};
	hipLaunchKernelGGL(k_sim3_scan, dim3((ns + 63) / 64), dim3(64), 0, st, sa);
	if (wantInliers) {
		HIPCHK(hipMemsetAsync(dVb, 0, b->sumN1, st));
		if (b->nc)
			hipLaunchKernelGGL(k_sim3_inliers, dim3((b->nc + 255) / 256), dim3(256), 0, st, b->nc, (const int*)b->dCorrSolver, (const int*)b->dIndex1,
			                   (const Sim3Solver*)b->dSolvers, (const Sim3Out*)dOut, (const unsigned long long*)ev.masks, dVb);
	}
	HIPCHK(hipGetLastError());
	if (int r = stg.finish(MCS_OK)) return r;
	for (int s = 0; s < ns; ++s) {
		const Sim3Out& o = b->hOut[s];
		b->mnIt[s] = o.mnIterations;
		success[s] = (uint8_t)o.success; no_more[s] = (uint8_t)o.noMore; n_inliers[s] = o.nInliers;
		if (T12 && o.success) memcpy(T12 + 16 * (size_t)s, o.T12, 128);   // `result` is written only on success
	}
	return MCS_OK;
}

int mcs_sim3_best(mcs_sim3* b, double* R, double* t, double* s, double* T12, int32_t* best_inliers, int32_t* iterations) {
	if (!b) return fail(MCS_ERR_INVALID, "null argument");
	if (!b->ns) return MCS_OK;
	HIPCHK(hipSetDevice(b->ctx->device));
	std::vector<Sim3State> hs(b->ns);
	HIPCHK(hipMemcpyAsync(hs.data(), b->dState, sizeof(Sim3State) * b->ns, hipMemcpyDeviceToHost, b->ctx->stream));
	HIPCHK(hipStreamSynchronize(b->ctx->stream));
	for (int k = 0; k < b->ns; ++k) {
		const Sim3State& x = hs[k];
		if (R) memcpy(R + 9 * (size_t)k, x.bestR, 72);
		if (t) memcpy(t + 3 * (size_t)k, x.bestt, 24);
		if (s) s[k] = x.bestS;
		if (T12) memcpy(T12 + 16 * (size_t)k, x.bestT12, 128);
		if (best_inliers) best_inliers[k] = x.mnBestInliers;
		if (iterations) iterations[k] = x.mnIterations;
	}
	return MCS_OK;
}

int mcs_sim3_hypotheses(mcs_sim3* b, int solver, int first, int count, int32_t* picks, int32_t* n_inliers, double* hyp, uint8_t* inliers) {
	if (!b || solver < 0 || solver >= b->ns || first < 0 || count < 0) return fail(MCS_ERR_INVALID, "bad argument");
	if (count && !n_inliers) return fail(MCS_ERR_INVALID, "null n_inliers");
	const Sim3Solver S = b->solvers[solver];
	if (count && S.N < 3) return fail(MCS_ERR_INVALID, "mcs_sim3_hypotheses: the solver has fewer than 3 correspondences");
	if (S.drawOff >= 0 && (long long)first + count > S.nDraws) return fail(MCS_ERR_INVALID, "mcs_sim3_hypotheses: beyond the caller's draws");
	if (!count) return MCS_OK;
	HIPCHK(hipSetDevice(b->ctx->device));
	std::vector<Sim3Slot> slots;
	long long words = 0;
	add_slots(b, solver, first, count, slots, words);
	std::vector<unsigned long long> m(inliers ? (size_t)words : 0);
	Staging stg(b->ctx, true);
	Eval ev{};
	eval_stage(stg, slots, words, ev, hyp, picks, inliers ? m.data() : nullptr, n_inliers);
	if (int r = stg.commit()) return r;
	if (int r = stg.finish(eval_launch(b, slots.size(), ev))) return r;
	if (inliers)
		for (int h = 0; h < count; ++h)
			for (int i = 0; i < S.N; ++i) inliers[(size_t)h * S.N + i] = (uint8_t)((m[(size_t)h * S.maskWords + (i >> 6)] >> (i & 63)) & 1ull);
	return MCS_OK;
}

int mcs_sim3_draw(uint64_t seed, int solver, int iteration, int pick, int n) {
	if (solver < 0 || iteration < 0 || pick < 0 || pick > 2 || n < 1) return -1;
	return sim3_draw(seed, solver, iteration, pick, n);
}
