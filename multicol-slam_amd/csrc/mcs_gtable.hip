// mcs_gtable.hip — the fast descriptor pass's per-camera table of G(s), its packed device form and the worst-case bound of the fast arithmetic against the
// reference's: host arithmetic only, in long double where the last places matter (tests/test_describe_bound_cpu.py pins them).
#include "mcs_extractor.h"

using namespace mcs;

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The fast pass's table of G(s) = rho(theta) / sqrt(s), theta = atan(p0 / sqrt(s)), for one camera (layout: mcs_common.h kG*), built in long double, with
// the bound on what its truncated Taylor rows leave out and the few magnitudes describe_fast_bound() needs (GTabInfo, mcs_extractor.h).
//
// Row (e, k): s = 2^e (kappa + tau), kappa = 1 + (k + 1/2) / 2^kGM, |tau| <= 2^-(kGM+1); centre c = 2^e kappa, eps = tau / kappa = (s - c) / c.
//   N(eps)      = (1 + eps)^(-1/2) = sum b_j eps^j                        (1 / sqrt(s) = N / sqrt(c))
//   z(eps)      = z_c N(eps),  z_c = p0 / sqrt(c);   y = z - z_c
//   atan(z_c+y) = theta_c + sum_k A_k y^k,  A_k from 1 / ((1 + z_c^2) + 2 z_c y + y^2)
//   rho         = sum_k p_k (theta - theta_c)^k,  p_k = invP re-expanded at theta_c
//   G           = N * rho / sqrt(c), truncated at eps^kGDeg, stored in the kernel's variable tau (coefficient j divided by kappa^j).
// Tail (coefficient-wise majorants, "<<"):  |b_j| <= 1/2 (j >= 1), so y << |z_c| (eps/2) / (1 - eps);  the Taylor coefficients of atan at the real point z_c
// are (1/k) Im-parts of (z_c -+ i)^-k, at most R^-k / k with R = sqrt(1 + z_c^2), so theta - theta_c << (Y/R) / (1 - Y/R) = a eps / (1 - b eps) with
// q = |z_c| / R, a = q / 2, b = 1 + q / 2;  rho - p_0 << sum_k |p_k| (a eps / (1 - b eps))^k, whose eps^i coefficient is P_i = sum_k |p_k| a^k b^(i-k) C(i-1, k-1);
// G << c^(-1/2) N~ (|p_0| + P) with N~ = sum |b_j| eps^j:  W_j = c^(-1/2) (|p_0| |b_j| + sum_{i=1..j} P_i |b_(j-i)|).  The truncated tail of a row is at most
// sum_{j > kGDeg} W_j epsmax^j (summed to j = 80; the rest is below c^(-1/2) (|p_0| + sum |p_k|) 3 (3 epsmax)^81 / (1 - 3 epsmax) since P_i <= sum|p_k| (2b)^i, 2b <= 3).
// What the pixel coordinates see is sqrt(s) times that: tailU.

// The packed device form of a table (mcs_common.h kGDev*): per row [g0 g1 g2 g3] as doubles, [g4 g5 g6 0] as floats (round to nearest).
void mcs::pack_g_table(const double* tab, uint8_t* out) {
	for (int r = 0; r < kGRows; ++r) {
		double* d = reinterpret_cast<double*>(out + (size_t)r * kGDevRowBytes);
		const double* g = tab + (size_t)r * kGRow;
		d[0] = g[0]; d[1] = g[1]; d[2] = g[2]; d[3] = g[3];
		float* f = reinterpret_cast<float*>(d + 4);
		f[0] = (float)g[4]; f[1] = (float)g[5]; f[2] = (float)g[6]; f[3] = 0.f;
	}
}

GTabInfo mcs::build_g_table(const mcs_ocam& m, double* tab) {
	typedef long double LD;
	GTabInfo info;
	const int n = m.invP_deg, D = kGDeg, J = 80;
	if (n < 1 || n > MCS_MAX_POLY || !(std::fabs(m.p[0]) > 1e-300) || !std::isfinite(m.p[0])) return info;
	for (int i = 0; i < n; ++i) if (!std::isfinite(m.invP[i])) return info;
	LD binom[MCS_MAX_POLY][MCS_MAX_POLY];
	for (int i = 0; i < MCS_MAX_POLY; ++i)
		for (int k = 0; k <= i; ++k) binom[i][k] = (k == 0 || k == i) ? 1.0L : binom[i - 1][k - 1] + binom[i - 1][k];
	LD bj[J + 1];   // (1 + eps)^(-1/2)
	bj[0] = 1.0L;
	for (int j = 1; j <= J; ++j) bj[j] = bj[j - 1] * (-(LD)(2 * j - 1) / (LD)(2 * j));
	auto mul = [&](const LD* A, const LD* B, LD* C) {   // series product truncated at degree D
		LD T[D + 1];
		for (int i = 0; i <= D; ++i) { T[i] = 0; for (int k = 0; k <= i; ++k) T[i] += A[k] * B[i - k]; }
		for (int i = 0; i <= D; ++i) C[i] = T[i];
	};
	const LD p0 = (LD)m.p[0];
	auto direct = [&](LD sv) {   // G(s) itself
		const LD nn = sqrtl(sv), th = atanl(p0 / nn);
		LD r = 0;
		for (int i = n - 1; i >= 0; --i) r = r * th + (LD)m.invP[i];
		return r / nn;
	};
	double tailU = 0, rhoB = 0, dB = 0, lip = 0, inB = 0, seen = 0, f32U = 0;
	for (int e = kGE0; e < kGE1; ++e)
		for (int k = 0; k < (1 << kGM); ++k) {
			const LD kappa = 1.0L + ((LD)k + 0.5L) / (LD)(1 << kGM), c = ldexpl(kappa, e), sqc = sqrtl(c), zc = p0 / sqc, thc = atanl(zc);
			const double epsmax = (double)(ldexpl(1.0L, -(kGM + 1)) / kappa) * (1.0 + 1e-15);
			// y(eps), atan coefficients, composition
			LD y[D + 1], A[D + 1], f[D + 1];
			y[0] = 0;
			for (int j = 1; j <= D; ++j) y[j] = zc * bj[j];
			const LD d0 = 1.0L + zc * zc;
			f[0] = 1.0L / d0;
			for (int j = 1; j <= D; ++j) f[j] = -(2.0L * zc * f[j - 1] + (j >= 2 ? f[j - 2] : 0.0L)) / d0;
			for (int j = 1; j <= D; ++j) A[j] = f[j - 1] / (LD)j;
			LD Th[D + 1] = {0}, Yp[D + 1];
			for (int j = 0; j <= D; ++j) Yp[j] = y[j];
			for (int kk = 1; kk <= D; ++kk) {
				for (int j = 0; j <= D; ++j) Th[j] += A[kk] * Yp[j];
				mul(Yp, y, Yp);
			}
			LD pk[MCS_MAX_POLY];
			for (int kk = 0; kk < n; ++kk) {
				LD acc = 0.0L, pw = 1.0L;
				for (int j = kk; j < n; ++j) { acc += binom[j][kk] * (LD)m.invP[j] * pw; pw *= thc; }
				pk[kk] = acc;
			}
			LD H[D + 1] = {0};
			H[0] = pk[n - 1];
			for (int kk = n - 2; kk >= 0; --kk) { mul(H, Th, H); H[0] += pk[kk]; }
			LD Gs[D + 1], Nn[D + 1];
			for (int j = 0; j <= D; ++j) Nn[j] = bj[j];
			mul(Nn, H, Gs);
			double* row = tab + (size_t)((e - kGE0) * (1 << kGM) + k) * kGRow;
			LD kp = 1.0L;
			for (int j = 0; j <= D; ++j) {
				Gs[j] /= sqc;
				row[j] = (double)(Gs[j] / kp);
				kp *= kappa;
				if (!std::isfinite(row[j])) return info;
			}
			// the majorant series W_j and the row's tail
			const double q = (double)(fabsl(zc) / sqrtl(d0)), a = 0.5 * q, b = 1.0 + 0.5 * q;
			double apk[MCS_MAX_POLY], Spk = 0;
			for (int kk = 0; kk < n; ++kk) { apk[kk] = (double)fabsl(pk[kk]) * (1.0 + 1e-15); if (kk) Spk += apk[kk]; }
			double P[J + 1];
			P[0] = 0;
			for (int i = 1; i <= J; ++i) {
				double acc = 0, cb = 1.0;   // cb = C(i-1, kk-1)
				for (int kk = 1; kk < n && kk <= i; ++kk) { acc += apk[kk] * std::pow(a, kk) * std::pow(b, i - kk) * cb; cb = cb * (double)(i - kk) / (double)kk; }
				P[i] = acc;
			}
			const double isc = (double)(1.0L / sqc) * (1.0 + 1e-15);
			double tail = 0, tailD = 0, ep = 1.0;   // sum W_j eps^j and sum j W_j eps^(j-1) over j > D
			for (int j = 1; j <= J; ++j) {
				const double epm1 = ep;
				ep *= epsmax;
				if (j <= D) continue;
				double Wj = apk[0] * (double)fabsl(bj[j]);
				for (int i = 1; i <= j; ++i) Wj += P[i] * (double)fabsl(bj[j - i]);
				Wj *= isc;
				tail += Wj * ep;
				tailD += (double)j * Wj * epm1;
			}
			const double rest = isc * (apk[0] + Spk) * 3.0 * std::pow(3.0 * epsmax, J + 1) / (1.0 - 3.0 * epsmax);
			tail = (tail + rest) * 1.01;                        // the sums above are in rounded arithmetic
			tailD = (tailD + (J + 2) * rest / epsmax) * 1.01;
			if (!std::isfinite(tail) || !std::isfinite(tailD)) return info;
			double gabs = 0, gder = 0;
			ep = 1.0;
			for (int j = 0; j <= D; ++j) {
				gabs += (double)fabsl(Gs[j]) * ep;
				if (j + 1 <= D) gder += (double)(j + 1) * (double)fabsl(Gs[j + 1]) * ep;
				ep *= epsmax;
			}
			gabs += tail;
			gder = (gder + tailD) * (1.0 + epsmax);             // |s G'(s)| = |(1 + eps) dG/d eps|
			const double sq = (double)sqc * std::sqrt(1.0 + epsmax) * (1.0 + 1e-15);
			tailU = std::max(tailU, sq * tail);
			rhoB = std::max(rhoB, sq * gabs);
			dB = std::max(dB, sq * gder);
			lip = std::max(lip, gabs + 2.0 * gder);
			inB = std::max(inB, (gabs + 2.0 * gder) * (sq + 44.0));
			// The float tail of the packed rows: T = g4 + g5 tau + g6 tau^2 with g_j and tau rounded to float and two float FMAs — the g6 term meets five
			// relative perturbations of 2^-24 (its coefficient, tau twice, both FMAs), g5 four, g4 two: |T_float - T| <= 6 * 2^-24 * sum |g_j| |tau|^(j-4) (the 6
			// and the 1.01 cover the second-order terms); T enters G as T tau^4, the coordinates as sqrt(s) G.  |tau| <= 2^-(kGM+1) in the kernel's variable.
			// Coefficients that do not fit a float make the table unusable; below the smallest normal float they are worth less than 1e-37 anyway (added).
			{
				const double tm = std::ldexp(1.0, -(kGM + 1));
				double t4 = 0, tp = tm * tm * tm * tm;
				for (int j = 4; j <= D; ++j) {
					if (!(std::fabs(row[j]) < 3.0e38) || !std::isfinite((double)(float)row[j])) return info;
					t4 += std::fabs(row[j]) * tp;
					tp *= tm;
				}
				f32U = std::max(f32U, sq * (6.0 * 1.01 * std::ldexp(1.0, -24) * t4 + 1e-37));
			}
			// sanity: the row against G itself at both ends of the bin and in the middle
			for (int t = -2; t <= 2; ++t) {
				const LD tau = (LD)t * ldexpl(1.0L, -(kGM + 2)) * (1.0L - 1e-9L), sv = ldexpl(kappa + tau, e);
				LD pv = 0;
				for (int j = D; j >= 0; --j) pv = pv * tau + (LD)row[j];
				seen = std::max(seen, (double)(fabsl(pv - direct(sv)) * sqrtl(sv)));
			}
		}
	info.f32U = f32U * 1.01;
	info.tailU = tailU; info.rhoB = rhoB * 1.01; info.dB = dB * 1.01; info.lip = lip * 1.01; info.inB = inB * 1.01; info.seen = seen;
	if (!(seen <= tailU + 64 * 1.1102230246251565e-16 * rhoB)) info.tailU = INFINITY;   // the rows must reproduce G within the bound they claim (plus their own rounding to double)
	return info;
}

// Worst-case |(fast coordinate - fast mean) - (reference coordinate - reference mean)| for one camera and npoints pattern points.
// u = 2^-53.  Both arithmetics evaluate the same real function F(X, Y) = affine(X G(s), Y G(s)), s = X^2 + Y^2, of the same real rotated pattern point
// (X, Y) = R(angle) (ptx, pty) + undistorted keypoint; each differs from it by its own rounding:
//   inputs  X = ptx ax - pty ay + ukx: reference 3 roundings, fast 2 (two FMAs), each relative to |ptx ax| + |pty ay| + |ukx| <= n + 44 for a point at distance
//           n from the axis (the keypoint lies within n + 22 of it, the rotated offset within 22).  F moves by at most aff * (|G| + 2 |s G'|) per unit of
//           either input; the product with n + 44 is maximised over the table's rows (inB): near the axis G ~ rho(axis) / n is large where n + 44 is small.
//   fast    s: 2 roundings (2.01 u relative, G moves by |s G'(s)| per relative unit: dB);  the row: truncated tail (tailU) + coefficients rounded to double +
//           6 FMAs (13 u of sum |g_j| |eps|^j: rhoB; the packed rows run 4 of them in double) + the float tail g4 .. g6 of the packed rows (f32U);  x G, y G: u
//           each;  the affine map without the principal point (it cancels against the mean): 2 more
//   ref     atan's argument and atan itself (12 u S' generously: ocml / glibc stay within 2 ulp) + 24 roundings of the Horner chain, 2 divisions, 2 products
//           (96 u S) + the affine map with the principal point (8 u (|u0| + |v0|));   S = sum |invP_i| (pi/2)^i,  S' = sum i |invP_i| (pi/2)^(i-1)
//   mean    the same per-point bound, plus the order of the sum: reference npoints - 1 sequential additions and a division, fast 2 NB - 1 per lane, 6 shuffle
//           levels and a product -> (npoints + 2 NB + 7) u Umax, Umax = 16384 + 4096 (enforced by the kernel)
//   minus   reference: one rounding of a value below 8192;  fast: the subtraction happens in fixed point (coordinate + (1.5 * 2^20 + 0.5 - mean), two
//           roundings of 2^-33 each)
// Returns +inf for a camera the fast arithmetic cannot serve (p0 = 0, non-finite coefficients, a table that fails its own check).
double mcs::describe_fast_bound(const mcs_ocam& m, int npoints, const GTabInfo& g) {
	const double u = 1.1102230246251565e-16, hp = 1.5707963267948966;
	double S = 0, Sp = 0, pw = 1.0;
	for (int i = 0; i < m.invP_deg; ++i) {
		if (!std::isfinite(m.invP[i])) return INFINITY;
		S += std::fabs(m.invP[i]) * pw;
		if (i + 1 < m.invP_deg) Sp += (i + 1) * std::fabs(m.invP[i + 1]) * pw;
		pw *= hp;
	}
	if (!(std::fabs(m.p[0]) > 1e-300) || !std::isfinite(m.p[0]) || !std::isfinite(g.tailU) || !std::isfinite(g.rhoB) || !std::isfinite(g.dB) || !std::isfinite(g.lip) || !std::isfinite(g.inB) || !std::isfinite(g.f32U)) return INFINITY;
	const double aff = 1.0 + std::fabs(m.c) + std::fabs(m.d) + std::fabs(m.e), pp = 8 * u * (std::fabs(m.u0) + std::fabs(m.v0));
	const int nb = npoints / 128;
	const double inputs = aff * g.inB * (2 * (2 + 3) * u * 1.01);
	const double fast = aff * (g.tailU + 16 * u * g.rhoB + 2.01 * u * g.dB + g.f32U);
	const double ref = aff * (12 * u * Sp + 96 * u * S) + pp;
	const double point = inputs + fast + ref;
	const double total = 2 * point + (npoints + 2 * nb + 7) * u * 20480.0 + 2 * u * 8192.0 + 2.3283064365386963e-10 * 1.001;
	return std::isfinite(total) ? total : INFINITY;
}

extern "C" {

int mcs_describe_fast_bound(const mcs_ocam* cam, int desc_size, double* bound) {
	if (!cam || !bound || cam->invP_deg < 1 || cam->invP_deg > MCS_MAX_POLY || cam->p_deg < 1) return fail(MCS_ERR_INVALID, "bad argument");
	std::vector<double> tab(kGTabDoubles, 0.0);
	*bound = describe_fast_bound(*cam, 2 * 8 * desc_size, build_g_table(*cam, tab.data()));
	return MCS_OK;
}

int mcs_describe_fast_table(const mcs_ocam* cam, double* table, int* rows, int* row_len, int* e0, int* bins_per_octave, double* info6) {
	if (!cam || cam->invP_deg < 1 || cam->invP_deg > MCS_MAX_POLY || cam->p_deg < 1) return fail(MCS_ERR_INVALID, "bad argument");
	std::vector<double> tab(kGTabDoubles, 0.0);
	const GTabInfo g = build_g_table(*cam, tab.data());
	if (table) memcpy(table, tab.data(), tab.size() * sizeof(double));
	if (rows) *rows = kGRows;
	if (row_len) *row_len = kGRow;
	if (e0) *e0 = kGE0;
	if (bins_per_octave) *bins_per_octave = 1 << kGM;
	if (info6) { info6[0] = g.tailU; info6[1] = g.rhoB; info6[2] = g.dB; info6[3] = g.lip; info6[4] = g.seen; info6[5] = g.inB; }
	return MCS_OK;
}

int mcs_describe_fast_table_packed(const mcs_ocam* cam, void* packed, int* row_bytes, double* f32_term) {
	if (!cam || cam->invP_deg < 1 || cam->invP_deg > MCS_MAX_POLY || cam->p_deg < 1) return fail(MCS_ERR_INVALID, "bad argument");
	std::vector<double> tab(kGTabDoubles, 0.0);
	const GTabInfo g = build_g_table(*cam, tab.data());
	if (packed) pack_g_table(tab.data(), reinterpret_cast<uint8_t*>(packed));
	if (row_bytes) *row_bytes = kGDevRowBytes;
	if (f32_term) *f32_term = g.f32U;
	return MCS_OK;
}

}  // extern "C"
