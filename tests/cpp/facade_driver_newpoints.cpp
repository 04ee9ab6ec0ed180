// MultiColSLAM::CreateNewMapPoints of the C++ facade end to end: reads a rig, the current keyframe and its neighbours (keypoints, rays, descriptors, map
// points), runs the neighbour loop in one call and writes every output (tests/test_gpu_newpoints_facade.py).
#include "mcs/mcs_facade.hpp"

#include <unordered_map>

using namespace MultiColSLAM;

struct MP {
	Vec3d X;
	Vec3d GetWorldPos() { return X; }
};
struct KF {
	cMultiCamSys_ camSystem;
	std::unordered_map<size_t, int> keypoint_to_cam, cont_idx_to_local_cam_idx;
	std::vector<KeyPoint> keys;
	std::vector<Vec3d> rays;
	std::vector<std::vector<uint8_t>> desc;   // per camera, rows of dim bytes (the reference's mDescriptors)
	std::vector<MP> points;
	std::vector<MP*> mp;
	int dim = 32;
	std::vector<MP*> GetMapPointMatches() { return mp; }
	std::vector<KeyPoint> GetKeyPoints() { return keys; }
	std::vector<Vec3d> GetKeyPointsRays() { return rays; }
	const uint64_t* GetDescriptorRowPtr(int cam, int row) const { return reinterpret_cast<const uint64_t*>(&desc[cam][(size_t)row * dim]); }
	const uint64_t* GetDescriptorMaskRowPtr(int, int) const { return nullptr; }
};

template <class T>
static T rd(std::FILE* f) { T v; if (std::fread(&v, sizeof(T), 1, f) != 1) throw std::runtime_error("short input"); return v; }
template <class T>
static void rdn(std::FILE* f, T* p, size_t n) { if (n && std::fread(p, sizeof(T), n, f) != n) throw std::runtime_error("short input"); }

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	std::FILE* f = std::fopen(argv[1], "rb");
	if (!f) return 2;
	const int nr = rd<int32_t>(f), nkf = rd<int32_t>(f), dim = rd<int32_t>(f);
	std::vector<cCamModelGeneral_> models(nr);
	std::vector<Matx44d> Mc(nr);
	for (int c = 0; c < nr; ++c) {
		models[c].ocam = rd<mcs_ocam>(f);
		rdn(f, Mc[c].data(), 16);
	}
	std::vector<KF> kfs((size_t)nkf);
	for (KF& kf : kfs) {
		kf.camSystem.camModels = models;
		kf.camSystem.M_c = Mc;
		Matx44d Mt;
		rdn(f, Mt.data(), 16);
		kf.camSystem.Set_M_t(Mt);
		kf.dim = dim;
		const int n = rd<int32_t>(f);
		kf.keys.resize(n); kf.rays.resize(n); kf.points.resize(n); kf.mp.assign(n, nullptr);
		rdn(f, kf.keys.data(), (size_t)n);
		std::vector<int32_t> cam(n);
		rdn(f, cam.data(), (size_t)n);
		rdn(f, kf.rays.data(), (size_t)n);
		std::vector<uint8_t> d((size_t)n * dim), has(n);
		rdn(f, d.data(), d.size());
		rdn(f, has.data(), (size_t)n);
		std::vector<Vec3d> pos(n);
		rdn(f, pos.data(), (size_t)n);
		kf.desc.assign(nr, {});
		for (int i = 0; i < n; ++i) {
			kf.keypoint_to_cam[i] = cam[i];
			kf.cont_idx_to_local_cam_idx[i] = (int)(kf.desc[cam[i]].size() / dim);
			kf.desc[cam[i]].insert(kf.desc[cam[i]].end(), d.begin() + (size_t)i * dim, d.begin() + (size_t)(i + 1) * dim);
			if (has[i]) { kf.points[i].X = pos[i]; kf.mp[i] = &kf.points[i]; }
		}
	}
	std::fclose(f);
	Context ctx(0);
	std::vector<KF*> neigh;
	for (int s = 1; s < nkf; ++s) neigh.push_back(&kfs[s]);
	const NewMapPoints r = CreateNewMapPoints<KF, MP>(ctx, &kfs[0], neigh, false, dim);
	std::FILE* o = std::fopen(argv[2], "wb");
	if (!o) return 2;
	for (const NewMapPoints::Neighbour& nb : r.neighbours) {
		const int32_t head[4] = {(int32_t)nb.vMatchedIndices.size(), nb.nmatches, nb.fallbacks, nb.skipped};
		std::fwrite(head, 4, 4, o);
		std::fwrite(&nb.baseline, 8, 1, o);
		std::fwrite(&nb.medianDepth, 8, 1, o);
		std::fwrite(nb.match12.data(), 4, nb.match12.size(), o);
		std::fwrite(nb.verdict.data(), 4, nb.verdict.size(), o);
		for (size_t k = 0; k < nb.vMatchedIndices.size(); ++k) {
			const int32_t p[2] = {(int32_t)nb.vMatchedIndices[k].first, (int32_t)nb.vMatchedIndices[k].second};
			std::fwrite(p, 4, 2, o);
			std::fwrite(nb.x3D[k].v, 8, 3, o);
		}
	}
	std::fwrite(r.valid1.data(), 1, r.valid1.size(), o);
	std::fclose(o);
	return 0;
}
