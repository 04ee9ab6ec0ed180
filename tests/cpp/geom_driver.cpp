// The host side of csrc/mcs_geom.h alone (tests/test_geom_cpu.py): no HIP call, no device.
//   geom_driver <in> <out>
// in : int32 nrCams, n, nvec, sizeof(mcs_ocam), useMasks; double pose[6]; double McMin[nrCams][6]; mcs_ocam cams[nrCams];
//      useMasks ? uint8 masks[nrCams][height * width] : nothing; double pts[n][3]; int32 pcam[n];
//      double a[nvec][3], b[nvec][3], M3[nvec][9], M4[nvec][16]
// out: double Mt[16], Mc[nrCams][16], MtMcInv[nrCams][16], uv[n][2]; uint8 flags[n] (bit 0 in the mirror mask, bit 1 behind);
//      double dot[nvec], norm[nvec], mv3[nvec][3] (ld = 3), mv4[nvec][3] (ld = 4)
#include "mcs_geom.h"
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

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	const std::vector<int> h = get<int>(in, 5);
	const int nr = h[0], n = h[1], nvec = h[2];
	if (h[3] != (int)sizeof(mcs_ocam)) { fprintf(stderr, "sizeof(mcs_ocam) = %zu\n", sizeof(mcs_ocam)); return 5; }
	const std::vector<double> pose = get<double>(in, 6), mcMin = get<double>(in, 6 * (size_t)nr);
	const std::vector<mcs_ocam> cams = get<mcs_ocam>(in, nr);
	std::vector<std::vector<uint8_t> > masks(nr);
	if (h[4]) for (int c = 0; c < nr; ++c) masks[c] = get<uint8_t>(in, (size_t)cams[c].width * cams[c].height);
	const std::vector<double> pts = get<double>(in, 3 * (size_t)n);
	const std::vector<int> pcam = get<int>(in, n);
	const std::vector<double> a = get<double>(in, 3 * (size_t)nvec), b = get<double>(in, 3 * (size_t)nvec), M3 = get<double>(in, 9 * (size_t)nvec),
	                          M4 = get<double>(in, 16 * (size_t)nvec);

	std::vector<double> Mt(16), Mc(16 * (size_t)nr), inv(16 * (size_t)nr), uv(2 * (size_t)n);
	std::vector<uint8_t> flags(n);
	cayley2hom(pose.data(), Mt.data());
	std::vector<OcamDev> dev(nr);
	for (int c = 0; c < nr; ++c) {   // Set_M_t_from_min: MtMc_inv[c] = invMat(M_t * M_c[c])
		double MtMc[16];
		cayley2hom(mcMin.data() + 6 * c, Mc.data() + 16 * c);
		matx44_mul(Mt.data(), Mc.data() + 16 * c, MtMc);
		inv_mat(MtMc, inv.data() + 16 * c);
		dev[c] = ocam_dev_of(cams[c]);
	}
	for (int i = 0; i < n; ++i) {
		const int c = pcam[i];
		double u, v;
		const bool behind = world_to_cam_hom_fast(inv.data() + 16 * c, dev[c], pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], u, v);
		uv[2 * i] = u; uv[2 * i + 1] = v;
		flags[i] = (uint8_t)((in_mirror_mask(u, v, cams[c].width, cams[c].height, h[4] ? masks[c].data() : nullptr) ? 1 : 0) | (behind ? 2 : 0));
	}
	std::vector<double> dot(nvec), nrm(nvec), mv3(3 * (size_t)nvec), mv4(3 * (size_t)nvec);
	for (int i = 0; i < nvec; ++i) {
		dot[i] = dot3(a.data() + 3 * i, b.data() + 3 * i);
		nrm[i] = norm3(a.data() + 3 * i);
		mat3_vec3(M3.data() + 9 * i, 3, a.data() + 3 * i, mv3.data() + 3 * i);
		mat3_vec3(M4.data() + 16 * i, 4, a.data() + 3 * i, mv4.data() + 3 * i);
	}
	put(out, Mt); put(out, Mc); put(out, inv); put(out, uv); put(out, flags); put(out, dot); put(out, nrm); put(out, mv3); put(out, mv4);
	fclose(in);
	return fclose(out) == 0 ? 0 : 4;
}
