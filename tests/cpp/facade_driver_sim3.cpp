// MultiColSLAM::cSim3Solver of the C++ facade end to end: reads a rig, two keyframe poses and the matched map points of one loop candidate, runs the
// loop closer's SetRansacParameters(0.98, 15, 300) + iterate(50) rounds and writes every call's outputs and the estimate (tests/test_gpu_sim3_facade.py).
#include "mcs/mcs_facade.hpp"

#include <unordered_map>

using namespace MultiColSLAM;

struct MP;
struct KP { int octave; };
struct KF {
	cMultiCamSys_ camSystem;
	std::unordered_map<size_t, int> keypoint_to_cam;
	std::vector<MP*> mp;
	std::vector<KP> kps;
	std::vector<double> sigma2;
	std::vector<MP*> GetMapPointMatches() { return mp; }
	const KP& GetKeyPoint(int i) const { return kps[i]; }
	double GetSigma2(int l) const { return sigma2[l]; }
};
struct MP {
	Vec3d X;
	std::vector<size_t> idx;
	KF* kf;
	bool isBad() { return false; }
	std::vector<size_t> GetIndexInKeyFrame(KF* k) { return k == kf ? idx : std::vector<size_t>{}; }
	Vec3d GetWorldPos() { return X; }
};

template <class T>
static T rd(std::FILE* f) { T v; if (std::fread(&v, sizeof(T), 1, f) != 1) throw std::runtime_error("short input"); return v; }

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	std::FILE* f = std::fopen(argv[1], "rb");
	if (!f) return 2;
	const int nr = rd<int32_t>(f), n = rd<int32_t>(f), mN1 = rd<int32_t>(f);
	const uint64_t seed = rd<uint64_t>(f);
	std::vector<cCamModelGeneral_> models(nr);
	std::vector<Matx44d> Mc(nr);
	for (int c = 0; c < nr; ++c) {
		mcs_ocam& o = models[c].ocam;
		o = rd<mcs_ocam>(f);
		for (int k = 0; k < 16; ++k) Mc[c][k] = rd<double>(f);
	}
	KF kf[2];
	std::vector<double> sig(8);
	for (int l = 0; l < 8; ++l) sig[l] = rd<double>(f);
	for (int s = 0; s < 2; ++s) {
		kf[s].camSystem.camModels = models;
		kf[s].camSystem.M_c = Mc;
		Matx44d Mt;
		for (int k = 0; k < 16; ++k) Mt[k] = rd<double>(f);
		kf[s].camSystem.Set_M_t(Mt);
		kf[s].sigma2 = sig;
		kf[s].mp.assign(mN1, nullptr);
		kf[s].kps.resize(mN1);
	}
	std::vector<MP> pts(2 * (size_t)mN1);
	std::vector<MP*> matches(mN1, nullptr);
	for (int i = 0; i < n; ++i) {
		const int i1 = rd<int32_t>(f);
		for (int s = 0; s < 2; ++s) {
			MP& p = pts[2 * (size_t)i1 + s];
			for (int k = 0; k < 3; ++k) p.X.v[k] = rd<double>(f);
			const int cam = rd<int32_t>(f), oct = rd<int32_t>(f);
			p.kf = &kf[s];
			p.idx = {(size_t)i1};   // feature i1 in both keyframes
			kf[s].keypoint_to_cam[i1] = cam;
			kf[s].kps[i1].octave = oct;
			kf[s].mp[i1] = &p;
		}
		matches[i1] = &pts[2 * (size_t)i1 + 1];
	}
	std::fclose(f);
	Context ctx(0);
	cSim3Solver<KF, MP> solver(ctx, &kf[0], &kf[1], matches, &kf[0].camSystem, seed);
	solver.SetRansacParameters(0.98, 15, 300);
	std::FILE* o = std::fopen(argv[2], "wb");
	if (!o) return 2;
	for (int call = 0; call < 50; ++call) {
		bool noMore = false;
		std::vector<bool> vb;
		int ni = -1;
		Matx44d T{};
		const bool ok = solver.iterate(50, noMore, vb, ni, T);
		const int32_t head[3] = {ok, noMore, ni};
		std::fwrite(head, 4, 3, o);
		std::vector<uint8_t> b(vb.begin(), vb.end());
		std::fwrite(b.data(), 1, b.size(), o);
		std::fwrite(T.data(), 8, 16, o);
		if (ok || noMore) break;
	}
	const std::array<double, 9> R = solver.GetEstimatedRotation();
	const Vec3d t = solver.GetEstimatedTranslation();
	const double s = solver.GetEstimatedScale();
	std::fwrite(R.data(), 8, 9, o);
	std::fwrite(t.v, 8, 3, o);
	std::fwrite(&s, 8, 1, o);
	std::fclose(o);
	return 0;
}
