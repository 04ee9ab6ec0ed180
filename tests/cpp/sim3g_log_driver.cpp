// The host side of csrc/mcs_sim3g.h's log, 3x3 LU and edge error alone (tests/test_sim3g_log_cpu.py): no HIP call, no device.
//   sim3g_log_driver <in> <out>
// in : int32 nlog, nedge, nlu; double S[nlog][8]; double CSiSj[nedge][24] (the measurement, vertex i, the INVERSE of vertex j); double Wb[nlu][12] (W row-major, b)
// a Sim3 of 8 is in operator[] order: qx qy qz qw tx ty tz s
// out: double log[nlog][10] (the seven, the branch, the pivot rows of columns 0 and 1), edge[nedge][7], lu[nlu][5] (x, the pivot rows)
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
static Sim3g load(const double* p) {
	Sim3g S;
	for (int k = 0; k < 4; ++k) S.q[k] = p[k];
	for (int k = 0; k < 3; ++k) S.t[k] = p[4 + k];
	S.s = p[7];
	return S;
}

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	const std::vector<int> h = get<int>(in, 3);
	const std::vector<double> S = get<double>(in, 8 * (size_t)h[0]), ed = get<double>(in, 24 * (size_t)h[1]), wb = get<double>(in, 12 * (size_t)h[2]);
	std::vector<double> o;
	for (int i = 0; i < h[0]; ++i) {
		double r[7];
		int br = -1, piv[2] = {-1, -1};
		sim3_log(load(&S[8 * (size_t)i]), r, &br, piv);
		o.insert(o.end(), r, r + 7);
		o.push_back((double)br); o.push_back((double)piv[0]); o.push_back((double)piv[1]);
	}
	for (int i = 0; i < h[1]; ++i) {
		double r[7];
		const double* p = &ed[24 * (size_t)i];
		sim3_edge_error(load(p), load(p + 8), load(p + 16), r);
		o.insert(o.end(), r, r + 7);
	}
	for (int i = 0; i < h[2]; ++i) {
		double W[9], x[3];
		int piv[2] = {-1, -1};
		for (int k = 0; k < 9; ++k) W[k] = wb[12 * (size_t)i + k];
		lu3_solve(W, &wb[12 * (size_t)i + 9], x, piv);
		o.insert(o.end(), x, x + 3);
		o.push_back((double)piv[0]); o.push_back((double)piv[1]);
	}
	if (!o.empty() && fwrite(o.data(), sizeof(double), o.size(), out) != o.size()) return 4;
	fclose(in);
	return fclose(out) == 0 ? 0 : 4;
}
