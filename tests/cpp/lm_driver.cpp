// The host side of csrc/mcs_lm.h and of the optimisers' derivatives in csrc/mcs_geom.h alone (tests/test_lm_cpu.py): no HIP call, no device.
//   lm_driver <in> <out>
// in : int32 n6, n7, nrCams, sizeof(mcs_ocam), npts, nposes, nhuber, nlm;
//      n6 x double Hu[21], lambda, b[6], x[6];  n7 x double Hu[28], lambda, b[7], x[7];
//      mcs_ocam cams[nrCams]; double McMin[nrCams][6]; double pts[npts][3]; int32 pcam[npts]; double poses[nposes][6];
//      double huber[nhuber][3] (c2, delta, dsqr);
//      nlm x { double state[7] (lambda, ni, currentChi, iniChi, postChi, lastChi, rho), chi, lambda0 (< 0: tau * max |H_jj| of Hu), Hu[21], maxDiag0,
//              trial[10][2] (rawChi, scale); int32 qmax, lmBad, it, postAlways, cap, ntrials, solveOk[10] }
// out: n6 x { double x[6], ok }; n7 x { double x[7], ok }; double dInvP[nrCams][MCS_MAX_POLY]; double D[npts][6]; double A[nposes][nrCams][27];
//      double rho[nhuber][2]; nlm x { double state[7]; int32 qmax, lmBad, nrun, end, stop, accepted[10] }
// An iteration of the table runs as the kernels run it: lm_iter_begin, lm_start at iteration 0, then lm_trial / lm_more until the loop ends or the row's
// trials run out, then lm_iter_end and the terminate action.  postAlways: postChi is written before the acceptance test (the essential graph), else on
// acceptance.  cap: the action stops without a test from this iteration on (the essential graph: 15; none: a large number).  stop: 1 the gain test, 2 the cap.
#include "mcs_geom.h"
#include "mcs_lm.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mcs;

template <class T>
static std::vector<T> get(FILE* f, size_t n) {
	std::vector<T> v(n);
	if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(3); }
	return v;
}
template <class T>
static void put(FILE* f, const std::vector<T>& v) {
	if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short output\n"); exit(4); }
}

template <int N>
static void solves(FILE* in, FILE* out, int n) {
	constexpr int T = N * (N + 1) / 2;
	for (int i = 0; i < n; ++i) {
		const std::vector<double> v = get<double>(in, T + 1 + 2 * N);
		std::vector<double> r(v.begin() + T + 1 + N, v.end());
		const bool ok = ldlt_solve<N>(v.data(), v[T], v.data() + T + 1, r.data());
		r.push_back(ok ? 1.0 : 0.0);
		put(out, r);
	}
}

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	const std::vector<int> h = get<int>(in, 8);
	const int nr = h[2], npts = h[4], nposes = h[5], nhuber = h[6], nlm = h[7];
	if (h[3] != (int)sizeof(mcs_ocam)) { fprintf(stderr, "sizeof(mcs_ocam) = %zu\n", sizeof(mcs_ocam)); return 5; }
	solves<6>(in, out, h[0]);
	solves<7>(in, out, h[1]);

	const std::vector<mcs_ocam> cams = get<mcs_ocam>(in, nr);
	const std::vector<double> mcMin = get<double>(in, 6 * (size_t)nr), pts = get<double>(in, 3 * (size_t)npts);
	const std::vector<int> pcam = get<int>(in, npts);
	const std::vector<double> poses = get<double>(in, 6 * (size_t)nposes);
	std::vector<OcamDev> dev(nr);
	std::vector<double> dInvP((size_t)nr * MCS_MAX_POLY), D(6 * (size_t)npts), A(27 * (size_t)nposes * nr);
	for (int c = 0; c < nr; ++c) {
		dev[c] = ocam_dev_of(cams[c]);
		ocam_dinvp(cams[c], dev[c], dInvP.data() + (size_t)c * MCS_MAX_POLY);
	}
	for (int i = 0; i < npts; ++i) {
		double d[2][3];
		d_world_to_img(dev[pcam[i]], dInvP.data() + (size_t)pcam[i] * MCS_MAX_POLY, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], d);
		for (int k = 0; k < 6; ++k) D[6 * (size_t)i + k] = d[k / 3][k % 3];
	}
	for (int p = 0; p < nposes; ++p)
		for (int c = 0; c < nr; ++c) {
			double Mt[16], McH[16];
			cayley2hom(poses.data() + 6 * p, Mt);
			cayley2hom(mcMin.data() + 6 * c, McH);
			cayley_rot_factors(poses.data() + 6 * p, Mt, McH, A.data() + 27 * ((size_t)p * nr + c));
		}
	put(out, dInvP); put(out, D); put(out, A);

	const std::vector<double> hub = get<double>(in, 3 * (size_t)nhuber);
	std::vector<double> rho(2 * (size_t)nhuber);
	for (int i = 0; i < nhuber; ++i) huber_robustify(hub[3 * i], hub[3 * i + 1], hub[3 * i + 2], rho[2 * i], rho[2 * i + 1]);
	put(out, rho);

	for (int i = 0; i < nlm; ++i) {
		const std::vector<double> v = get<double>(in, 7 + 2 + 21 + 1 + 20);
		const std::vector<int> q = get<int>(in, 6 + 10);
		LmState s{v[0], v[1], v[2], v[3], v[4], v[5], v[6], q[0], q[1]};
		const int it = q[2], postAlways = q[3], cap = q[4], ntrials = q[5];
		const double* trial = v.data() + 31;
		std::vector<int> r(5 + 10, 0);
		lm_iter_begin(s, v[7]);
		if (it == 0) lm_start(s, v[8] < 0 ? lm_lambda_init(max_abs_diag<6>(v.data() + 9, v[30])) : v[8]);
		int k = 0;
		while (k < ntrials) {
			const double raw = trial[2 * k];
			if (postAlways) s.postChi = raw;
			const bool acc = lm_trial(s, raw, q[6 + k] != 0, trial[2 * k + 1]);
			if (acc && !postAlways) s.postChi = raw;
			r[5 + k] = acc ? 1 : 0;
			++k;
			if (!lm_more(s)) break;
		}
		r[2] = k;
		r[3] = lm_iter_end(s);
		if (it < cap) r[4] = lm_gain_stop(s, it) ? 1 : 0;
		else r[4] = 2;
		r[0] = s.qmax; r[1] = s.lmBad;
		put(out, std::vector<double>{s.lambda, s.ni, s.currentChi, s.iniChi, s.postChi, s.lastChi, s.rho});
		put(out, r);
	}
	fclose(in);
	return fclose(out) == 0 ? 0 : 4;
}
