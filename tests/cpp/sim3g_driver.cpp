// The host side of csrc/mcs_sim3g.h alone (tests/test_sim3g_cpu.py): no HIP call, no device.
//   sim3g_driver <in> <out>
// in : int32 nexp, nrts, nmul, ninv, nmap, nmat; double u[nexp][7]; double rts[nrts][13] (R row-major, t, s); double ab[nmul][16] (two Sim3 of 8);
//      double S[ninv][8]; double Sx[nmap][11] (a Sim3, a point); double q[nmat][4]
// a Sim3 of 8 is in operator[] order: qx qy qz qw tx ty tz s
// out: double exp[nexp][9] (the Sim3, then the branch), rts[nrts][8], mul[nmul][8], inv[ninv][8], map[nmap][3], rot[nmap][3] (the quaternion alone),
//      mat[nmat][9], conj[nmat][4]
#include "mcs_sim3g.h"
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
static void put(FILE* f, const std::vector<double>& v) {
	if (!v.empty() && fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) { fprintf(stderr, "short output\n"); exit(4); }
}
static Sim3g load(const double* p) {
	Sim3g S;
	for (int k = 0; k < 4; ++k) S.q[k] = p[k];
	for (int k = 0; k < 3; ++k) S.t[k] = p[4 + k];
	S.s = p[7];
	return S;
}
static void store(const Sim3g& S, std::vector<double>& o) {
	for (int k = 0; k < 4; ++k) o.push_back(S.q[k]);
	for (int k = 0; k < 3; ++k) o.push_back(S.t[k]);
	o.push_back(S.s);
}

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	const std::vector<int> h = get<int>(in, 6);
	const std::vector<double> u = get<double>(in, 7 * (size_t)h[0]), rts = get<double>(in, 13 * (size_t)h[1]), ab = get<double>(in, 16 * (size_t)h[2]),
	                          si = get<double>(in, 8 * (size_t)h[3]), sx = get<double>(in, 11 * (size_t)h[4]), q = get<double>(in, 4 * (size_t)h[5]);
	std::vector<double> o;
	for (int i = 0; i < h[0]; ++i) { int br = -1; store(sim3_exp(&u[7 * (size_t)i], &br), o); o.push_back((double)br); }
	for (int i = 0; i < h[1]; ++i) store(sim3_from_rts(&rts[13 * (size_t)i], &rts[13 * (size_t)i + 9], rts[13 * (size_t)i + 12]), o);
	for (int i = 0; i < h[2]; ++i) store(sim3_mul(load(&ab[16 * (size_t)i]), load(&ab[16 * (size_t)i + 8])), o);
	for (int i = 0; i < h[3]; ++i) store(sim3_inverse(load(&si[8 * (size_t)i])), o);
	for (int i = 0; i < h[4]; ++i) { double r[3]; sim3_map(load(&sx[11 * (size_t)i]), &sx[11 * (size_t)i + 8], r); o.insert(o.end(), r, r + 3); }
	for (int i = 0; i < h[4]; ++i) { double r[3]; quat_rotate(&sx[11 * (size_t)i], &sx[11 * (size_t)i + 8], r); o.insert(o.end(), r, r + 3); }
	for (int i = 0; i < h[5]; ++i) { double R[9]; quat_to_mat(&q[4 * (size_t)i], R); o.insert(o.end(), R, R + 9); }
	for (int i = 0; i < h[5]; ++i) { double r[4]; quat_conj(&q[4 * (size_t)i], r); o.insert(o.end(), r, r + 4); }
	put(out, o);
	fclose(in);
	return fclose(out) == 0 ? 0 : 4;
}
