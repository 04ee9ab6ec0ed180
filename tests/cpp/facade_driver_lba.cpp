// facade_driver_lba.cpp — MultiColSLAM::cOptimizer::LocalBundleAdjustment of include/mcs/mcs_facade.hpp on a little map read from a text file, over a rig
// loaded by LoadMCS.  usage: facade_driver_lba <calibration dir> <scene file>.  Scene file: nk, then per keyframe "mnId bad" and the 6 numbers of its
// Get_M_t_min(); nn and the nn neighbours of keyframe 0 (the current one) as indices; use_flag flag; nlevels and mvInvLevelSigma2; per keyframe nf and nf lines
// "x y octave cam point" (point: index or -1); np and np lines "X Y Z bad".  A point is observed where a feature holds it.
// Prints (hex floats): the length of the returned list and the flag; per keyframe its M_t_min; per point "X Y Z bad"; per keyframe one character per feature
// (1 = it still holds its point).
#include "mcs/mcs_facade.hpp"

#include <cstdio>
#include <fstream>
#include <map>

using namespace MultiColSLAM;

struct KeyFrame;
struct MapPoint {
	double X[3] = {0, 0, 0};
	bool bad = false;
	std::map<KeyFrame*, std::vector<size_t>> obs;
	const double* GetWorldPos() const { return X; }
	void SetWorldPos(const double* p) { X[0] = p[0]; X[1] = p[1]; X[2] = p[2]; }
	bool isBad() const { return bad; }
	void SetBadFlag() { bad = true; }
	const std::map<KeyFrame*, std::vector<size_t>>& GetObservations() const { return obs; }
	void EraseObservation(KeyFrame* k, size_t idx) {
		auto it = obs.find(k);
		if (it != obs.end()) it->second.erase(std::remove(it->second.begin(), it->second.end(), idx), it->second.end());
	}
};
struct KeyFrame {
	long unsigned int mnId = 0;
	bool bad = false;
	cMultiCamSys_ camSystem;
	std::vector<KeyPoint> mvKeys;
	std::map<size_t, int> keypoint_to_cam;
	std::vector<MapPoint*> mvpMapPoints;
	std::vector<KeyFrame*> neighbours;
	std::vector<double> mvInvLevelSigma2;
	bool isBad() const { return bad; }
	std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() const { return neighbours; }
	std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
	const KeyPoint& GetKeyPoint(size_t i) const { return mvKeys[i]; }
	void EraseMapPointMatch(size_t i) { mvpMapPoints[i] = nullptr; }
};

int main(int argc, char** argv) {
	if (argc != 3) { std::fprintf(stderr, "usage: %s <calibration dir> <scene file>\n", argv[0]); return 2; }
	cMultiCamSys_ rig;
	LoadMCS(argv[1], rig);
	std::ifstream in(argv[2]);
	size_t nk = 0, nn = 0, nlevels = 0, np = 0;
	in >> nk;
	std::vector<KeyFrame> kf(nk);
	for (KeyFrame& k : kf) {
		std::array<double, 6> m;
		in >> k.mnId >> k.bad;
		for (double& v : m) in >> v;
		k.camSystem = rig;
		k.camSystem.Set_M_t_from_min(m);
	}
	in >> nn;
	for (size_t i = 0; i < nn; ++i) { size_t j = 0; in >> j; kf[0].neighbours.push_back(&kf[j]); }
	int useFlag = 0;
	bool flag = false;
	in >> useFlag >> flag >> nlevels;
	std::vector<double> is2(nlevels);
	for (double& v : is2) in >> v;
	std::vector<std::vector<long>> held(nk);
	for (size_t k = 0; k < nk; ++k) {
		size_t nf = 0;
		in >> nf;
		kf[k].mvInvLevelSigma2 = is2;
		kf[k].mvKeys.resize(nf);
		held[k].resize(nf);
		for (size_t i = 0; i < nf; ++i) {
			KeyPoint& p = kf[k].mvKeys[i];
			int cam = 0;
			p = KeyPoint{};
			in >> p.ptx >> p.pty >> p.octave >> cam >> held[k][i];
			kf[k].keypoint_to_cam[i] = cam;
		}
	}
	in >> np;
	std::vector<MapPoint> pts(np);
	for (MapPoint& p : pts) in >> p.X[0] >> p.X[1] >> p.X[2] >> p.bad;
	if (!in) { std::fprintf(stderr, "bad scene file\n"); return 3; }
	for (size_t k = 0; k < nk; ++k)
		for (size_t i = 0; i < held[k].size(); ++i) {
			MapPoint* mp = held[k][i] < 0 ? nullptr : &pts[(size_t)held[k][i]];
			kf[k].mvpMapPoints.push_back(mp);
			if (mp) mp->obs[&kf[k]].push_back(i);
		}
	Context ctx(0);
	const std::list<KeyFrame*> ret = cOptimizer::LocalBundleAdjustment(ctx, &kf[0], useFlag ? &flag : nullptr);
	std::printf("%zu %d\n", ret.size(), flag ? 1 : 0);
	for (const KeyFrame& k : kf) {
		for (double v : k.camSystem.M_t_min) std::printf(" %a", v);
		std::printf("\n");
	}
	for (const MapPoint& p : pts) std::printf("%a %a %a %d\n", p.X[0], p.X[1], p.X[2], p.bad ? 1 : 0);
	for (const KeyFrame& k : kf) {
		for (MapPoint* m : k.mvpMapPoints) std::printf("%d", m ? 1 : 0);
		std::printf("\n");
	}
	return 0;
}
