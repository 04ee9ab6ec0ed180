// MultiColSLAM::SearchByProjectionLastFrame and MultiColSLAM::WindowSearchFrames of the C++ facade end to end: reads a rig (with mirror masks), the map points
// (position, bad flag) and two frames (keypoints, cameras, descriptors, the map point each feature holds, outlier flags), runs one of the two functions and
// writes its return value and, per feature of the second frame, the map point it holds afterwards (tests/test_gpu_lastframe_facade.py).
#include "mcs/mcs_facade.hpp"

#include <unordered_map>

using namespace MultiColSLAM;

struct MP {
	Vec3d X;
	bool bad = false;
	Vec3d GetWorldPos() { return X; }
	bool isBad() { return bad; }
};
struct FR {
	cMultiCamSys_ camSystem;
	std::unordered_map<size_t, int> keypoint_to_cam, cont_idx_to_local_cam_idx;
	std::vector<KeyPoint> mvKeys;
	std::vector<MP*> mvpMapPoints;
	std::vector<bool> mvbOutlier;
	std::vector<double> mvScaleFactors;
	std::vector<std::vector<uint8_t>> desc, mask;   // per camera, rows of dim bytes (the reference's mDescriptors / mDescriptorMasks)
	int dim = 32;
	const uint64_t* GetDescriptorRowPtr(int cam, int row) const { return reinterpret_cast<const uint64_t*>(&desc[cam][(size_t)row * dim]); }
	const uint64_t* GetDescriptorMaskRowPtr(int cam, int row) const { return reinterpret_cast<const uint64_t*>(&mask[cam][(size_t)row * dim]); }
};

template <class T>
static T rd(std::FILE* f) { T v; if (std::fread(&v, sizeof(T), 1, f) != 1) throw std::runtime_error("short input"); return v; }
template <class T>
static void rdn(std::FILE* f, T* p, size_t n) { if (n && std::fread(p, sizeof(T), n, f) != n) throw std::runtime_error("short input"); }

// n, keys, cameras, descriptors, masks, held point per feature (-1 none), outlier flags
static void read_frame(std::FILE* f, FR& F, int nr, int dim, std::vector<MP>& pts) {
	const int n = rd<int32_t>(f);
	F.dim = dim;
	F.mvKeys.resize(n);
	rdn(f, F.mvKeys.data(), (size_t)n);
	std::vector<int32_t> cam(n), held(n);
	std::vector<uint8_t> d((size_t)n * dim), m((size_t)n * dim), out(n);
	rdn(f, cam.data(), (size_t)n);
	rdn(f, d.data(), d.size()); rdn(f, m.data(), m.size());
	rdn(f, held.data(), (size_t)n); rdn(f, out.data(), (size_t)n);
	F.desc.assign(nr, {}); F.mask.assign(nr, {});
	F.mvpMapPoints.assign(n, nullptr);
	F.mvbOutlier.assign(n, false);
	for (int i = 0; i < n; ++i) {
		F.keypoint_to_cam[i] = cam[i];
		F.cont_idx_to_local_cam_idx[i] = (int)(F.desc[cam[i]].size() / dim);
		F.desc[cam[i]].insert(F.desc[cam[i]].end(), d.begin() + (size_t)i * dim, d.begin() + (size_t)(i + 1) * dim);
		F.mask[cam[i]].insert(F.mask[cam[i]].end(), m.begin() + (size_t)i * dim, m.begin() + (size_t)(i + 1) * dim);
		if (held[i] >= 0) F.mvpMapPoints[i] = &pts[held[i]];
		F.mvbOutlier[i] = out[i] != 0;
	}
}

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	std::FILE* f = std::fopen(argv[1], "rb");
	if (!f) return 2;
	const int nr = rd<int32_t>(f), dim = rd<int32_t>(f), nlevels = rd<int32_t>(f), withMirror = rd<int32_t>(f), havingMasks = rd<int32_t>(f);
	const int checkOri = rd<int32_t>(f), window = rd<int32_t>(f), windowSize = rd<int32_t>(f), minLevel = rd<int32_t>(f), maxLevel = rd<int32_t>(f);
	const double th = rd<double>(f), nnratio = rd<double>(f);
	FR Last, Cur;
	Cur.camSystem.camModels.resize(nr);
	Cur.camSystem.M_c.resize(nr);
	for (int c = 0; c < nr; ++c) {
		cCamModelGeneral_& m = Cur.camSystem.camModels[c];
		m.ocam = rd<mcs_ocam>(f);
		rdn(f, Cur.camSystem.M_c[c].data(), 16);
		if (withMirror) { m.mirrorMask0.create(m.ocam.height, m.ocam.width); rdn(f, m.mirrorMask0.data, (size_t)m.ocam.width * m.ocam.height); }
	}
	Matx44d Mt;
	rdn(f, Mt.data(), 16);
	Cur.camSystem.Set_M_t(Mt);
	Cur.mvScaleFactors.resize(nlevels);
	rdn(f, Cur.mvScaleFactors.data(), (size_t)nlevels);
	Last.mvScaleFactors = Cur.mvScaleFactors;
	const int np = rd<int32_t>(f);
	std::vector<MP> pts((size_t)np);
	for (MP& p : pts) { p.X = rd<Vec3d>(f); p.bad = rd<int32_t>(f) != 0; }
	read_frame(f, Last, nr, dim, pts);
	read_frame(f, Cur, nr, dim, pts);
	std::fclose(f);
	Context ctx(0);
	int32_t ret;
	std::vector<MP*> held;
	if (window) {
		ret = WindowSearchFrames<FR, MP>(ctx, Last, Cur, windowSize, held, minLevel, maxLevel, nnratio, dim, havingMasks != 0, checkOri != 0);
	} else {
		ret = SearchByProjectionLastFrame<FR, MP>(ctx, Cur, Last, th, dim, havingMasks != 0, checkOri != 0);
		held = Cur.mvpMapPoints;
	}
	std::FILE* o = std::fopen(argv[2], "wb");
	if (!o) return 2;
	std::fwrite(&ret, 4, 1, o);
	for (size_t i = 0; i < held.size(); ++i) { const int32_t k = held[i] ? (int32_t)(held[i] - pts.data()) : -1; std::fwrite(&k, 4, 1, o); }
	std::fclose(o);
	return 0;
}
