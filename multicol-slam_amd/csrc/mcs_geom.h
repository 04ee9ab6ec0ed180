// mcs_geom.h — the rig geometry of the map-side kernels (mcs_project / mcs_frustum / mcs_lastframe / mcs_newpoints / mcs_sim3 / mcs_poseopt / mcs_lba), stated once.
// Each function restates one statement of the reference's scalar C++ and is held to it bit for bit: FP64, no contraction, every sum in the reference's order.
// Host and device: tests/test_geom_cpu.py compiles this header alone for the host and compares it with the reference's compiled code.
#pragma once
#include "mcs_common.h"
#include <math.h>

#define MCS_GEOM __host__ __device__ __forceinline__

namespace mcs {

// ---------------------------------------------------------------------------------------------- cv::Matx / cv::Vec arithmetic as OpenCV 3.x performs it
// (modules/core/include/opencv2/core/matx.hpp and operations.hpp: every product and dot is "s = 0; s += a * b" in increasing k)

// Matx::dot / Vec::dot
MCS_GEOM double dot3(const double* a, const double* b) {
	double s = 0;
	for (int k = 0; k < 3; ++k) s += a[k] * b[k];
	return s;
}
// cv::norm(Vec3d): sqrt(((0 + a0^2) + a1^2) + a2^2)
MCS_GEOM double norm3(const double* v) { return sqrt(dot3(v, v)); }

// Matx33d * Vec3d; M is a row-major 3x3 (ld = 3) or the top-left 3x3 of a 4x4 (ld = 4)
MCS_GEOM void mat3_vec3(const double* M, int ld, const double* p, double* r) {
	for (int i = 0; i < 3; ++i) {
		double s = 0;
		for (int k = 0; k < 3; ++k) s += M[ld * i + k] * p[k];
		r[i] = s;
	}
}
// rows [0, Rows) of Matx44d * Vec4d
template <int Rows>
MCS_GEOM void matx44_vec4(const double* M, const double* p4, double* r) {
	static_assert(Rows == 3 || Rows == 4, "a camera-frame point or a homogeneous one");
	for (int i = 0; i < Rows; ++i) {
		double s = 0;
		for (int k = 0; k < 4; ++k) s += M[4 * i + k] * p4[k];
		r[i] = s;
	}
}
// ... of Matx44d * Vec4d(X(0), X(1), X(2), 1.0)
template <int Rows>
MCS_GEOM void matx44_point(const double* M, const double* X, double* r) {
	const double p4[4] = {X[0], X[1], X[2], 1.0};
	matx44_vec4<Rows>(M, p4, r);
}
// Matx44d * Matx44d
MCS_GEOM void matx44_mul(const double* A, const double* B, double* C) {
	for (int i = 0; i < 4; ++i)
		for (int j = 0; j < 4; ++j) {
			double s = 0;
			for (int k = 0; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j];
			C[4 * i + j] = s;
		}
}
// cConverter::invMat (src/cConverter.cpp:31-44): R^T and (-R^T) * t; `out` must not alias M
MCS_GEOM void inv_mat(const double* M, double* out) {
	for (int i = 0; i < 3; ++i) {
		double s = 0;
		for (int k = 0; k < 3; ++k) { out[4 * i + k] = M[4 * k + i]; s += (-M[4 * k + i]) * M[4 * k + 3]; }
		out[4 * i + 3] = s;
	}
	out[12] = out[13] = out[14] = 0.0; out[15] = 1.0;
}

// ---------------------------------------------------------------------------------------------- Cayley parameters (include/misc.h)
// cayley2rot, :133-160
MCS_GEOM void cayley2rot(const double* c, double* R) {
	const double c1 = c[0], c2 = c[1], c3 = c[2];
	const double c1s = c1 * c1, c2s = c2 * c2, c3s = c3 * c3;
	const double scale = 1.0 + c1s + c2s + c3s;
	R[0] = 1 + c1s - c2s - c3s; R[1] = 2 * (c1 * c2 - c3);   R[2] = 2 * (c1 * c3 + c2);
	R[3] = 2 * (c1 * c2 + c3);  R[4] = 1 - c1s + c2s - c3s;  R[5] = 2 * (c2 * c3 - c1);
	R[6] = 2 * (c1 * c3 - c2);  R[7] = 2 * (c2 * c3 + c1);   R[8] = 1 - c1s - c2s + c3s;
	const double inv = 1 / scale;
	for (int k = 0; k < 9; ++k) R[k] = inv * R[k];
}
// cayley2hom, :212-224
MCS_GEOM void cayley2hom(const double* c6, double* M) {
	double R[9];
	cayley2rot(c6, R);
	for (int r = 0; r < 3; ++r) { M[4 * r] = R[3 * r]; M[4 * r + 1] = R[3 * r + 1]; M[4 * r + 2] = R[3 * r + 2]; M[4 * r + 3] = c6[3 + r]; }
	M[12] = M[13] = M[14] = 0.0; M[15] = 1.0;
}

// ---------------------------------------------------------------------------------------------- the camera
// mcs_ocam -> the kernels' camera model, on the device: invP zero-extended to MCS_MAX_POLY (horner_fixed), every other field set (the forward polynomial is
// not carried: no map-side kernel goes from the image to a ray).  The host's checked form is ocam_to_dev (mcs_host.h).
MCS_GEOM OcamDev ocam_dev_of(const mcs_ocam& m) {
	OcamDev o;
	o.c = m.c; o.d = m.d; o.e = m.e; o.u0 = m.u0; o.v0 = m.v0; o.invAffine = m.c - m.d * m.e;
	const int deg = m.invP_deg < 0 ? 0 : m.invP_deg > MCS_MAX_POLY ? MCS_MAX_POLY : m.invP_deg;
	for (int k = 0; k < MCS_MAX_POLY; ++k) { o.p[k] = 0.0; o.invP[k] = k < deg ? m.invP[k] : 0.0; }
	o.p_deg = 0; o.invP_deg = deg; o.fastOk = 0; o.tabIdx = 0;
	return o;
}

// include/misc.h:115-122 (zero-padded fixed-length form, see mcs_describe.hip)
MCS_GEOM double horner_fixed(const double* coeffs, double x) {
	double res = 0.0;
#pragma unroll
	for (int i = MCS_MAX_POLY - 1; i >= 0; i--) res = res * x + coeffs[i];
	return res;
}

// cCamModelGeneral_::WorldToImg (src/cam_model_omni.cpp:146-161)
MCS_GEOM void omni_world_to_img(const OcamDev& cam, double x, double y, double z, double& u, double& v) {
	double norm = sqrt(x * x + y * y);
	if (norm == 0.0) norm = 1e-14;
	const double theta = atan(-z / norm);
	const double rho = horner_fixed(cam.invP, theta);
	const double uu = x / norm * rho;
	const double vv = y / norm * rho;
	u = uu * cam.c + vv * cam.d + cam.u0;
	v = uu * cam.e + vv + cam.v0;
}

// ---------------------------------------------------------------------------------------------- the derivatives of the optimisers (mcs_poseopt / mcs_lba.hip)
// Derived here by the chain rule — the reference's Jacobians are generated text and are not used in any form — and held bit for bit to the same statements
// of tests/poseopt_model.py (d_world_to_img, d_cayley2rot) by tests/test_lm_cpu.py.

// the coefficients of d rho / d theta for horner_fixed: k * invP[k], zero behind the degree
MCS_GEOM void ocam_dinvp(const mcs_ocam& m, const OcamDev& o, double* dInvP) {
	for (int k = 0; k < MCS_MAX_POLY; ++k) dInvP[k] = k + 1 < o.invP_deg ? m.invP[k + 1] * (double)(k + 1) : 0.0;
}

// d(u, v) / d(x, y, z) of omni_world_to_img; the norm == 0 -> 1e-14 branch is a constant
MCS_GEOM void d_world_to_img(const OcamDev& cam, const double* dInvP, double x, double y, double z, double D[2][3]) {
	const double n0 = sqrt(x * x + y * y);
	const bool constant = n0 == 0.0;
	const double n = constant ? 1e-14 : n0;
	const double dn[3] = {constant ? 0.0 : x / n, constant ? 0.0 : y / n, 0.0};
	const double q = -z / n;
	const double theta = atan(q);
	const double dthdq = 1.0 / (1.0 + q * q);
	const double rho = horner_fixed(cam.invP, theta), drho_dth = horner_fixed(dInvP, theta);
	const double fx = x / n, fy = y / n;
	for (int k = 0; k < 3; ++k) {
		const double dq = k == 2 ? -1.0 / n : (z / (n * n)) * dn[k];
		const double drho = drho_dth * (dthdq * dq);
		const double dfx = -(x / (n * n)) * dn[k] + (k == 0 ? 1.0 / n : 0.0);
		const double dfy = -(y / (n * n)) * dn[k] + (k == 1 ? 1.0 / n : 0.0);
		const double duu = dfx * rho + fx * drho, dvv = dfy * rho + fy * drho;
		D[0][k] = duu * cam.c + dvv * cam.d;
		D[1][k] = duu * cam.e + dvv;
	}
}

// A_i = Rc^T (dRt/dc_i)^T, i = 0..2, row-major 3x3 each: with Mct = Mt * Mc the camera-frame point is p = Rc^T Rt^T (X - t) - Rc^T tc, so
// dp/dc_i = A_i (X - t).  cayley2rot is R = N / s with s = 1 + |c|^2, so dR/dc_i = (dN/dc_i - 2 c_i R) / s.  Mt = cayley2hom(pose), McH = cayley2hom(M_c_min[c]).
MCS_GEOM void cayley_rot_factors(const double* pose, const double* Mt, const double* McH, double* A) {
	const double c1 = pose[0], c2 = pose[1], c3 = pose[2];
	const double s = 1.0 + c1 * c1 + c2 * c2 + c3 * c3;
	const double dN[3][9] = {{2 * c1, 2 * c2, 2 * c3, 2 * c2, -2 * c1, -2.0, 2 * c3, 2.0, -2 * c1},
	                         {-2 * c2, 2 * c1, 2.0, 2 * c1, 2 * c2, 2 * c3, -2.0, 2 * c3, -2 * c2},
	                         {-2 * c3, -2.0, 2 * c1, 2.0, -2 * c3, 2 * c2, 2 * c1, 2 * c2, 2 * c3}};
	for (int i = 0; i < 3; ++i) {
		double dR[9];
		for (int k = 0; k < 9; ++k) dR[k] = (dN[i][k] - 2.0 * pose[i] * Mt[4 * (k / 3) + k % 3]) / s;
		for (int r = 0; r < 3; ++r)
			for (int k = 0; k < 3; ++k) {
				double a = 0;
				for (int j = 0; j < 3; ++j) a += McH[4 * j + r] * dR[3 * k + j];
				A[9 * i + 3 * r + k] = a;
			}
	}
}

// cCamModelGeneral_::isPointInMirrorMask(u, v, 0) (src/cam_model_omni.cpp:163-178): cvRound, the open bounds test, then the level-0 mask (nullptr: bounds only).
// cvRound is cvtsd2si on x86-64: round-half-even, and INT_MIN for a NaN or a rounded value outside int.  The device's conversion saturates instead (NaN -> 0,
// +-huge -> INT_MAX / INT_MIN); the open bounds test rejects 0, INT_MIN and INT_MAX alike (W <= INT_MAX), so both give the same answer for every double
// (DESIGN.md section 7).  The host branch states the x86 rule — not (int)lrint, which keeps the low 32 bits of a long and would let 2^32 + 5 in; it serves
// the CPU tests only.
MCS_GEOM int cv_round_host(double v) {
	const double r = nearbyint(v);
	return (r >= -2147483648.0 && r < 2147483648.0) ? (int)r : (-2147483647 - 1);
}
MCS_GEOM bool in_mirror_mask_at(int ur, int vr, int W, int H, const uint8_t* m) {
	if (ur >= W || ur <= 0 || vr >= H || vr <= 0) return false;
	return !m || m[(size_t)vr * W + ur] > 0;
}
MCS_GEOM bool in_mirror_mask(double u, double v, int W, int H, const uint8_t* m) {
#ifdef __HIP_DEVICE_COMPILE__
	return in_mirror_mask_at(__double2int_rn(u), __double2int_rn(v), W, H, m);
#else
	return in_mirror_mask_at(cv_round_host(u), cv_round_host(v), W, H, m);
#endif
}

// bool cMultiCamSys_::WorldToCamHom_fast(int c, pt, pt2) with M = MtMc_inv[c] (src/cam_system_omni.cpp:92-133, the flagMcMt branch): ptRot = M * pt, WorldToImg,
// and ptRot.z <= 0.  The Vec3d overload (:114-133) extends the point by 1.0 and returns nothing; the Vec4d overload (:92-112) multiplies the caller's fourth
// component, which CreateNewMapPoints computes (src/cLocalMapping.cpp:312-313, 323): that caller alone passes w.
MCS_GEOM bool world_to_cam_hom_fast(const double* M, const OcamDev& cam, double x, double y, double z, double& u, double& v, double w = 1.0) {
	const double p4[4] = {x, y, z, w};
	double r[3];
	matx44_vec4<3>(M, p4, r);
	omni_world_to_img(cam, r[0], r[1], r[2], u, v);
	return r[2] <= 0.0;
}

}  // namespace mcs
