// mcs_sim3g.h — the arithmetic of g2o::Sim3 (ThirdParty/g2o/g2o/types/sim3.h) and of the Eigen 3.2.10 quaternion it stands on
// (ThirdParty/Eigen/Eigen/src/Geometry/Quaternion.h), stated once for mcs_sim3opt.hip.  Each function restates the cited lines in their scalar form (no SSE
// path: an SSE2 build of the reference runs Eigen's vectorised quaternion product, which orders its operands differently): FP64, no contraction, every sum
// in the order Eigen's expression evaluates it.  Host and device: tests/test_sim3g_cpu.py compiles this header alone for the host and holds it bit for bit to
// tests/sim3opt_model.py.  log() and the edge error of the essential graph (mcs_essgraph.hip) follow at the end: tests/test_sim3g_log_cpu.py holds
// them to tests/essgraph_model.py in the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#ifndef MCS_GEOM
#define MCS_GEOM __host__ __device__ __forceinline__
#endif

namespace mcs {

// Quaterniond r (coeffs() order: x y z w), Vector3d t, double s: the members of g2o::Sim3, in the order of its operator[] (sim3.h:239-250)
struct Sim3g { double q[4]; double t[3]; double s; };

// the eight doubles of a Sim3 in memory (S12, Scw, Snc of include/mcs_c.h): q (x y z w), t, s
MCS_GEOM Sim3g sim3_load(const double* p) { Sim3g S; S.q[0] = p[0]; S.q[1] = p[1]; S.q[2] = p[2]; S.q[3] = p[3]; S.t[0] = p[4]; S.t[1] = p[5]; S.t[2] = p[6]; S.s = p[7]; return S; }
MCS_GEOM void sim3_store(const Sim3g& S, double* p) { p[0] = S.q[0]; p[1] = S.q[1]; p[2] = S.q[2]; p[3] = S.q[3]; p[4] = S.t[0]; p[5] = S.t[1]; p[6] = S.t[2]; p[7] = S.s; }

// Quaternion(const MatrixBase&) for a 3x3: quaternionbase_assign_impl<Other,3,3>::run (Quaternion.h:720-759), Shoemake.  R row-major.
// mat.trace() is diagonal().sum(): Eigen's unrolled scalar redux halves the range (Core/Redux.h:77-90), so it is m00 + (m11 + m22).
MCS_GEOM void quat_from_mat(const double* R, double* q) {
	double t = R[0] + (R[4] + R[8]);
	if (t > 0.0) {
		t = sqrt(t + 1.0);
		q[3] = 0.5 * t;
		t = 0.5 / t;
		q[0] = (R[7] - R[5]) * t;
		q[1] = (R[2] - R[6]) * t;
		q[2] = (R[3] - R[1]) * t;
	} else {
		int i = 0;
		if (R[4] > R[0]) i = 1;
		if (R[8] > R[4 * i]) i = 2;
		const int j = (i + 1) % 3, k = (j + 1) % 3;
		t = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
		q[i] = 0.5 * t;
		t = 0.5 / t;
		q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
		q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
		q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
	}
}

// quat_product<Arch, ...>::run, the generic form (Quaternion.h:419-430); out must not alias a or b
MCS_GEOM void quat_mul(const double* a, const double* b, double* out) {
	out[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
	out[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
	out[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
	out[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

// MatrixBase::cross for 3-vectors (Geometry/OrthoMethods.h:26-44)
MCS_GEOM void cross3(const double* a, const double* b, double* r) {
	r[0] = a[1] * b[2] - a[2] * b[1];
	r[1] = a[2] * b[0] - a[0] * b[2];
	r[2] = a[0] * b[1] - a[1] * b[0];
}

// QuaternionBase::_transformVector (Quaternion.h:462-474): uv = vec x v; uv += uv; v + w * uv + vec x uv.  The quaternion is NOT normalised here or anywhere.
MCS_GEOM void quat_rotate(const double* q, const double* v, double* r) {
	double uv[3], c[3];
	cross3(q, v, uv);
	for (int k = 0; k < 3; ++k) uv[k] += uv[k];
	cross3(q, uv, c);
	for (int k = 0; k < 3; ++k) r[k] = v[k] + q[3] * uv[k] + c[k];
}

// QuaternionBase::conjugate (Quaternion.h:655-660)
MCS_GEOM void quat_conj(const double* q, double* r) { r[0] = -q[0]; r[1] = -q[1]; r[2] = -q[2]; r[3] = q[3]; }

// QuaternionBase::toRotationMatrix (Quaternion.h:523-557); R row-major
MCS_GEOM void quat_to_mat(const double* q, double* R) {
	const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
	const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
	const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
	const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
	R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
	R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
	R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

// Sim3(const Matrix3d& R, const Vector3d& t, double s) (sim3.h:64-67)
MCS_GEOM Sim3g sim3_from_rts(const double* R, const double* t, double s) {
	Sim3g S;
	quat_from_mat(R, S.q);
	S.t[0] = t[0]; S.t[1] = t[1]; S.t[2] = t[2]; S.s = s;
	return S;
}

// Sim3(const Vector7d& update) (sim3.h:70-142): the exponential map, four branches on |sigma| < 1e-5 and theta < 1e-5.  omega.norm() is the square root of
// the halved redux w0^2 + (w1^2 + w2^2); a 3x3 product sums in increasing k; I + a * Omega + b * Omega2 adds left to right, entry by entry.
// branch (optional): 2 * (|sigma| >= eps) + (theta >= eps).
MCS_GEOM Sim3g sim3_exp(const double* u, int* branch = nullptr) {
	const double* w = u;
	const double* ups = u + 3;
	const double sigma = u[6];
	const double theta = sqrt(w[0] * w[0] + (w[1] * w[1] + w[2] * w[2]));
	const double Om[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};   // skew (se3_ops.hpp:27-38)
	Sim3g S;
	S.s = exp(sigma);
	double Om2[9], R[9];
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			double a = Om[3 * i] * Om[j];
			a += Om[3 * i + 1] * Om[3 + j];
			a += Om[3 * i + 2] * Om[6 + j];
			Om2[3 * i + j] = a;
		}
	const double eps = 0.00001;
	double A, B, C;
	bool series;   // R = I + Omega + Omega2 (:99, :117), else Rodrigues (:106, :121)
	if (fabs(sigma) < eps) {
		C = 1;
		if (theta < eps) { A = 1. / 2.; B = 1. / 6.; series = true; }
		else {
			const double theta2 = theta * theta;
			A = (1 - cos(theta)) / (theta2);
			B = (theta - sin(theta)) / (theta2 * theta);
			series = false;
		}
	} else {
		C = (S.s - 1) / sigma;
		if (theta < eps) {
			const double sigma2 = sigma * sigma;
			A = ((sigma - 1) * S.s + 1) / sigma2;
			B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
			series = true;
		} else {
			series = false;
			const double a = S.s * sin(theta);
			const double b = S.s * cos(theta);
			const double theta2 = theta * theta;
			const double sigma2 = sigma * sigma;
			const double c = theta2 + sigma2;
			A = (a * sigma + (1 - b) * theta) / (theta * c);
			B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
		}
	}
	if (branch) *branch = (fabs(sigma) < eps ? 0 : 2) + (theta < eps ? 0 : 1);
	if (series) {
		for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + Om[k]) + Om2[k];
	} else {
		const double ca = sin(theta) / theta, cb = (1 - cos(theta)) / (theta * theta);
		for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + ca * Om[k]) + cb * Om2[k];
	}
	quat_from_mat(R, S.q);
	double W[9];
	for (int k = 0; k < 9; ++k) W[k] = (A * Om[k] + B * Om2[k]) + C * (k % 4 == 0 ? 1.0 : 0.0);
	for (int i = 0; i < 3; ++i) {
		double a = W[3 * i] * ups[0];
		a += W[3 * i + 1] * ups[1];
		a += W[3 * i + 2] * ups[2];
		S.t[i] = a;
	}
	return S;
}

// Sim3::map (sim3.h:144-146): s * (r * xyz) + t
MCS_GEOM void sim3_map(const Sim3g& S, const double* x, double* r) {
	double v[3];
	quat_rotate(S.q, x, v);
	for (int k = 0; k < 3; ++k) r[k] = S.s * v[k] + S.t[k];
}

// Sim3::inverse (sim3.h:233-236): Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
MCS_GEOM Sim3g sim3_inverse(const Sim3g& S) {
	Sim3g I;
	quat_conj(S.q, I.q);
	const double f = -1. / S.s;
	const double v[3] = {f * S.t[0], f * S.t[1], f * S.t[2]};
	quat_rotate(I.q, v, I.t);
	I.s = 1. / S.s;
	return I;
}

// Sim3::operator* (sim3.h:266-272)
MCS_GEOM Sim3g sim3_mul(const Sim3g& a, const Sim3g& b) {
	Sim3g r;
	double v[3];
	quat_mul(a.q, b.q, r.q);
	quat_rotate(a.q, b.t, v);
	for (int k = 0; k < 3; ++k) r.t[k] = a.s * v[k] + a.t[k];
	r.s = a.s * b.s;
	return r;
}

// PartialPivLU of a 3x3 and its solve, as Eigen 3.2.10 runs W.lu().solve(t) for fixed size 3: partial_lu_impl::unblocked_lu (LU/PartialPivLU.h:245-287) — per
// column the FIRST largest |entry| at or below the diagonal (maxCoeff keeps the first), whole rows swapped, the column below divided by the pivot (a true
// division, Core/Functors.h:544), the corner updated by one product per entry; a zero column is left alone — then dst = P b, the unit-lower and the upper
// triangular solves unrolled (Core/SolveTriangular.h: x_i -= the sum of the products so far, two of them as a0 + a1; the upper one divides by the diagonal).
// W row-major, destroyed.  pivots (optional): the rows chosen for columns 0 and 1.
MCS_GEOM void lu3_solve(double* W, const double* b, double* x, int* pivots = nullptr) {
	double y[3] = {b[0], b[1], b[2]};
	for (int k = 0; k < 3; ++k) {
		int piv = k;
		double big = fabs(W[3 * k + k]);
		for (int r = k + 1; r < 3; ++r)
			if (fabs(W[3 * r + k]) > big) { big = fabs(W[3 * r + k]); piv = r; }
		if (pivots && k < 2) pivots[k] = piv;
		if (big != 0.0) {
			if (piv != k) {
				for (int c = 0; c < 3; ++c) { const double t = W[3 * k + c]; W[3 * k + c] = W[3 * piv + c]; W[3 * piv + c] = t; }
			}
			for (int r = k + 1; r < 3; ++r) W[3 * r + k] = W[3 * r + k] / W[3 * k + k];
		}
		if (piv != k) { const double t = y[k]; y[k] = y[piv]; y[piv] = t; }   // the transpositions applied to b in the order they were made
		for (int r = k + 1; r < 3; ++r)
			for (int c = k + 1; c < 3; ++c) W[3 * r + c] = W[3 * r + c] - W[3 * r + k] * W[3 * k + c];
	}
	y[1] -= W[3] * y[0];
	y[2] -= W[6] * y[0] + W[7] * y[1];
	x[2] = y[2] / W[8];
	x[1] = (y[1] - W[5] * x[2]) / W[4];
	x[0] = (y[0] - (W[1] * x[1] + W[2] * x[2])) / W[0];
}

// Sim3::log (sim3.h:148-230): four branches on |sigma| < 1e-5 and d > 1 - 1e-5 with d = 0.5 * (R00 + R11 + R22 - 1), left to right; deltaR and skew
// (se3_ops.hpp:27-49); W = A * Omega + B * Omega * Omega + C * I, where B * Omega * Omega is the product of (B * Omega) with Omega summed in increasing k;
// upsilon = W.lu().solve(t).  out: omega, upsilon, sigma.  branch (optional): 2 * (|sigma| >= eps) + (d <= 1 - eps).
MCS_GEOM void sim3_log(const Sim3g& S, double* out, int* branch = nullptr, int* pivots = nullptr) {
	const double sigma = log(S.s);
	double R[9];
	quat_to_mat(S.q, R);
	const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
	const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
	const double eps = 0.00001;
	const double s = S.s;
	double A, B, C, f;
	if (fabs(sigma) < eps) {
		C = 1;
		if (d > 1 - eps) { f = 0.5; A = 1. / 2.; B = 1. / 6.; }
		else {
			const double theta = acos(d);
			const double theta2 = theta * theta;
			f = theta / (2 * sqrt(1 - d * d));
			A = (1 - cos(theta)) / (theta2);
			B = (theta - sin(theta)) / (theta2 * theta);
		}
	} else {
		C = (s - 1) / sigma;
		if (d > 1 - eps) {
			const double sigma2 = sigma * sigma;
			f = 0.5;
			A = ((sigma - 1) * s + 1) / (sigma2);
			B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
		} else {
			const double theta = acos(d);
			f = theta / (2 * sqrt(1 - d * d));
			const double theta2 = theta * theta;
			const double a = s * sin(theta);
			const double b = s * cos(theta);
			const double c = theta2 + sigma * sigma;
			A = (a * sigma + (1 - b) * theta) / (theta * c);
			B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
		}
	}
	if (branch) *branch = (fabs(sigma) < eps ? 0 : 2) + (d > 1 - eps ? 0 : 1);
	const double w[3] = {f * dR[0], f * dR[1], f * dR[2]};
	const double Om[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
	double W[9];
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			double p = (B * Om[3 * i]) * Om[j];
			p += (B * Om[3 * i + 1]) * Om[3 + j];
			p += (B * Om[3 * i + 2]) * Om[6 + j];
			W[3 * i + j] = (A * Om[3 * i + j] + p) + C * (i == j ? 1.0 : 0.0);
		}
	lu3_solve(W, S.t, out + 3, pivots);
	out[0] = w[0]; out[1] = w[1]; out[2] = w[2];
	out[6] = sigma;
}

// edgeSim3::computeError (include/g2o_MultiCol_sim3_expmap.h:86-94): log(C * v1 * v2.inverse()), the products left to right; Sjinv is v2's inverse
MCS_GEOM void sim3_edge_error(const Sim3g& C, const Sim3g& Si, const Sim3g& Sjinv, double* e, int* branch = nullptr, int* pivots = nullptr) {
	sim3_log(sim3_mul(sim3_mul(C, Si), Sjinv), e, branch, pivots);
}

}  // namespace mcs
