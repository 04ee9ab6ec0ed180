// MultiColSLAM::SearchReferencePointsInFrustum of the C++ facade end to end: reads a rig (with mirror masks), the current frame (keypoints, descriptors,
// the map points it already holds) and the local map points with their tracking fields, runs the function and writes its return value, F.mvpMapPoints and
// every map point's fields and visible count (tests/test_gpu_frustum_facade.py).
#include "mcs/mcs_facade.hpp"

#include <unordered_map>

using namespace MultiColSLAM;

struct MP {
	Vec3d X, N;
	double minD = 0, maxD = 0;
	bool bad = false;
	long unsigned int mnLastFrameSeen = 0;
	int visible = 0;
	std::vector<bool> mbTrackInView;
	std::vector<double> mTrackProjX, mTrackProjY, mTrackViewCos;
	std::vector<int> mnTrackScaleLevel;
	std::vector<uint8_t> d, m;
	Vec3d GetWorldPos() { return X; }
	Vec3d GetNormal() { return N; }
	double GetMinDistanceInvariance() { return minD; }
	double GetMaxDistanceInvariance() { return maxD; }
	bool isBad() { return bad; }
	void IncreaseVisible() { ++visible; }
	const uint64_t* GetDescriptorPtr() { return reinterpret_cast<const uint64_t*>(d.data()); }
	const uint64_t* GetDescriptorMaskPtr() { return reinterpret_cast<const uint64_t*>(m.data()); }
};
struct FR {
	cMultiCamSys_ camSystem;
	long unsigned int mnId = 0;
	std::unordered_map<size_t, int> keypoint_to_cam, cont_idx_to_local_cam_idx;
	std::vector<KeyPoint> mvKeys;
	std::vector<MP*> mvpMapPoints;
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

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	std::FILE* f = std::fopen(argv[1], "rb");
	if (!f) return 2;
	const int nr = rd<int32_t>(f), dim = rd<int32_t>(f), nlevels = rd<int32_t>(f), withMirror = rd<int32_t>(f), havingMasks = rd<int32_t>(f);
	FR F;
	F.dim = dim;
	F.mnId = (long unsigned int)rd<int32_t>(f);
	F.camSystem.camModels.resize(nr);
	F.camSystem.M_c.resize(nr);
	for (int c = 0; c < nr; ++c) {
		cCamModelGeneral_& m = F.camSystem.camModels[c];
		m.ocam = rd<mcs_ocam>(f);
		rdn(f, F.camSystem.M_c[c].data(), 16);
		if (withMirror) { m.mirrorMask0.create(m.ocam.height, m.ocam.width); rdn(f, m.mirrorMask0.data, (size_t)m.ocam.width * m.ocam.height); }
	}
	Matx44d Mt;
	rdn(f, Mt.data(), 16);
	F.camSystem.Set_M_t(Mt);
	F.mvScaleFactors.resize(nlevels);
	rdn(f, F.mvScaleFactors.data(), (size_t)nlevels);
	// the local map points
	const int np = rd<int32_t>(f);
	std::vector<MP> pts((size_t)np);
	for (MP& p : pts) {
		p.X = rd<Vec3d>(f); p.N = rd<Vec3d>(f); p.minD = rd<double>(f); p.maxD = rd<double>(f);
		p.bad = rd<int32_t>(f) != 0; p.mnLastFrameSeen = (long unsigned int)rd<int32_t>(f);
		p.mbTrackInView.resize(nr); p.mTrackProjX.resize(nr); p.mTrackProjY.resize(nr); p.mTrackViewCos.resize(nr); p.mnTrackScaleLevel.resize(nr);
		for (int c = 0; c < nr; ++c) {
			p.mbTrackInView[c] = rd<int32_t>(f) != 0; p.mnTrackScaleLevel[c] = rd<int32_t>(f);
			p.mTrackProjX[c] = rd<double>(f); p.mTrackProjY[c] = rd<double>(f); p.mTrackViewCos[c] = rd<double>(f);
		}
		p.d.resize(dim); p.m.resize(dim);
		rdn(f, p.d.data(), (size_t)dim); rdn(f, p.m.data(), (size_t)dim);
	}
	// the frame; held[i] = index of the local map point feature i already holds, -1 none
	const int n = rd<int32_t>(f);
	F.mvKeys.resize(n);
	rdn(f, F.mvKeys.data(), (size_t)n);
	std::vector<int32_t> cam(n), held(n);
	rdn(f, cam.data(), (size_t)n);
	std::vector<uint8_t> d((size_t)n * dim), m((size_t)n * dim);
	rdn(f, d.data(), d.size()); rdn(f, m.data(), m.size());
	rdn(f, held.data(), (size_t)n);
	std::fclose(f);
	F.desc.assign(nr, {}); F.mask.assign(nr, {});
	F.mvpMapPoints.assign(n, nullptr);
	for (int i = 0; i < n; ++i) {
		F.keypoint_to_cam[i] = cam[i];
		F.cont_idx_to_local_cam_idx[i] = (int)(F.desc[cam[i]].size() / dim);
		F.desc[cam[i]].insert(F.desc[cam[i]].end(), d.begin() + (size_t)i * dim, d.begin() + (size_t)(i + 1) * dim);
		F.mask[cam[i]].insert(F.mask[cam[i]].end(), m.begin() + (size_t)i * dim, m.begin() + (size_t)(i + 1) * dim);
		if (held[i] >= 0) F.mvpMapPoints[i] = &pts[held[i]];
	}
	std::vector<MP*> local;
	for (MP& p : pts) local.push_back(&p);
	Context ctx(0);
	const int32_t ret = SearchReferencePointsInFrustum<FR, MP>(ctx, F, local, 3.0, 0.8, dim, havingMasks != 0);
	std::FILE* o = std::fopen(argv[2], "wb");
	if (!o) return 2;
	std::fwrite(&ret, 4, 1, o);
	for (int i = 0; i < n; ++i) { const int32_t k = F.mvpMapPoints[i] ? (int32_t)(F.mvpMapPoints[i] - pts.data()) : -1; std::fwrite(&k, 4, 1, o); }
	for (MP& p : pts) {
		const int32_t head[2] = {p.visible, (int32_t)p.mnLastFrameSeen};
		std::fwrite(head, 4, 2, o);
		for (int c = 0; c < nr; ++c) {
			const int32_t iv[2] = {p.mbTrackInView[c] ? 1 : 0, p.mnTrackScaleLevel[c]};
			const double dv[3] = {p.mTrackProjX[c], p.mTrackProjY[c], p.mTrackViewCos[c]};
			std::fwrite(iv, 4, 2, o); std::fwrite(dv, 8, 3, o);
		}
	}
	std::fclose(o);
	return 0;
}
