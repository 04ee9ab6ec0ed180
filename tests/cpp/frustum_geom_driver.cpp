// The host side of csrc/mcs_geom.h on the hostile rigs of tests/hostile_frustum.py (tests/test_frustum_hostile_cpu.py): no HIP call, no device.
//   frustum_geom_driver <in> <out>
// in : int32 nrCams, n, sizeof(mcs_ocam); mcs_ocam cams[nrCams]; double MtMcInv[nrCams][16]; per camera int32 hasMask, then hasMask ? uint8 mask[height * width]
//      : nothing; double pts[n][3]
// out: double uv[n][nrCams][2]; uint8 in[n][nrCams][3]: isPointInMirrorMask by
//      [0] in_mirror_mask's host branch (the x86 rule, cv_round_host),
//      [1] in_mirror_mask_at on a conversion that saturates as the device's __double2int_rn does (NaN -> 0, beyond int -> INT_MAX / INT_MIN),
//      [2] in_mirror_mask_at on (int)lrint(), which keeps the low 32 bits of a long: what the host branch was before, kept to show where it differs
#include "mcs_geom.h"
#include <climits>
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

static int saturating_rn(double v) {
	if (v != v) return 0;
	const double r = nearbyint(v);
	if (r >= 2147483648.0) return INT_MAX;
	if (r < -2147483648.0) return INT_MIN;
	return (int)r;
}

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	const std::vector<int> h = get<int>(in, 3);
	const int nr = h[0], n = h[1];
	if (h[2] != (int)sizeof(mcs_ocam)) { fprintf(stderr, "sizeof(mcs_ocam) = %zu\n", sizeof(mcs_ocam)); return 5; }
	const std::vector<mcs_ocam> cams = get<mcs_ocam>(in, nr);
	const std::vector<double> inv = get<double>(in, 16 * (size_t)nr);
	std::vector<std::vector<uint8_t> > masks(nr);
	std::vector<int> has(nr);
	for (int c = 0; c < nr; ++c) {
		has[c] = get<int>(in, 1)[0];
		if (has[c]) masks[c] = get<uint8_t>(in, (size_t)cams[c].width * cams[c].height);
	}
	const std::vector<double> pts = get<double>(in, 3 * (size_t)n);
	std::vector<double> uv(2 * (size_t)n * nr);
	std::vector<uint8_t> flags(3 * (size_t)n * nr);
	for (int i = 0; i < n; ++i)
		for (int c = 0; c < nr; ++c) {
			const size_t p = (size_t)i * nr + c;
			const uint8_t* m = has[c] ? masks[c].data() : nullptr;
			const int W = cams[c].width, H = cams[c].height;
			double u, v;
			(void)world_to_cam_hom_fast(inv.data() + 16 * c, ocam_dev_of(cams[c]), pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], u, v);
			uv[2 * p] = u; uv[2 * p + 1] = v;
			flags[3 * p] = in_mirror_mask(u, v, W, H, m) ? 1 : 0;
			flags[3 * p + 1] = in_mirror_mask_at(saturating_rn(u), saturating_rn(v), W, H, m) ? 1 : 0;
			flags[3 * p + 2] = in_mirror_mask_at((int)lrint(u), (int)lrint(v), W, H, m) ? 1 : 0;
		}
	put(out, uv); put(out, flags);
	fclose(in);
	return fclose(out) == 0 ? 0 : 4;
}
