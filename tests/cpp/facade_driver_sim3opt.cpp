// facade_driver_sim3opt.cpp — MultiColSLAM::cOptimizer::OptimizeSim3 of include/mcs/mcs_facade.hpp on two keyframes read from a text file, over a rig loaded
// by LoadMCS.  usage: facade_driver_sim3opt <calibration dir> <scene file>.  Scene file: 16 numbers M_t of keyframe 1, 16 of keyframe 2; R (9), t (3), s,
// stdSim; nlevels, the mvLevelSigma2 values, the mvInvLevelSigma2 values; n1 and n1 lines "x y octave cam" (the features of keyframe 1), n2 and n2 such lines;
// then n1 lines "X Y Z bad1  i2 X Y Z bad2": keyframe 1's point of feature i (bad1 = 2: NULL) and its match (i2 = -2: no match, vpMatches1[i] = NULL; -1: a match that
// keyframe 2 does not observe).  Prints (hex floats): the return value; q t s R of g2oS12 afterwards; one character per entry of vpMatches1 (1 = still set).
#include "mcs/mcs_facade.hpp"

#include <cstdio>
#include <fstream>
#include <map>

using namespace MultiColSLAM;

struct KeyFrame;
struct MapPoint {
	double X[3] = {0, 0, 0};
	bool bad = false;
	KeyFrame* kf = nullptr;
	int idx = -1;
	const double* GetWorldPos() const { return X; }
	bool isBad() const { return bad; }
	std::vector<int> GetIndexInKeyFrame(KeyFrame* k) const { return k == kf && idx >= 0 ? std::vector<int>{idx} : std::vector<int>{}; }
};
struct KeyFrame {
	cMultiCamSys_ camSystem;
	std::vector<KeyPoint> mvKeys;
	std::map<size_t, int> keypoint_to_cam;
	std::vector<MapPoint*> mvpMapPoints;
	std::vector<double> mvLevelSigma2, mvInvLevelSigma2;
	std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
	const KeyPoint& GetKeyPoint(size_t i) const { return mvKeys[i]; }
	double GetSigma2(int l) const { return mvLevelSigma2[(size_t)l]; }
	double GetInvSigma2(int l) const { return mvInvLevelSigma2[(size_t)l]; }
};

int main(int argc, char** argv) {
	if (argc != 3) { std::fprintf(stderr, "usage: %s <calibration dir> <scene file>\n", argv[0]); return 2; }
	cMultiCamSys_ rig;
	LoadMCS(argv[1], rig);
	std::ifstream in(argv[2]);
	KeyFrame kf[2];
	for (KeyFrame& k : kf) {
		k.camSystem = rig;
		Matx44d M;
		for (double& v : M) in >> v;
		k.camSystem.Set_M_t(M);
	}
	cOptimizer::Sim3 S;
	for (double& v : S.R) in >> v;
	for (double& v : S.t) in >> v;
	in >> S.s >> cOptimizer::stdSim();
	size_t nlevels = 0;
	in >> nlevels;
	std::vector<double> s2(nlevels), is2(nlevels);
	for (double& v : s2) in >> v;
	for (double& v : is2) in >> v;
	for (KeyFrame& k : kf) {
		k.mvLevelSigma2 = s2; k.mvInvLevelSigma2 = is2;
		size_t n = 0;
		in >> n;
		k.mvKeys.resize(n);
		for (size_t i = 0; i < n; ++i) {
			KeyPoint& p = k.mvKeys[i];
			int cam = 0;
			p = KeyPoint{};
			in >> p.ptx >> p.pty >> p.octave >> cam;
			k.keypoint_to_cam[i] = cam;
		}
	}
	const size_t n1 = kf[0].mvKeys.size();
	std::vector<MapPoint> p1(n1), p2(n1);
	std::vector<MapPoint*> vpMatches1(n1, nullptr);
	for (size_t i = 0; i < n1; ++i) {
		int i2 = -2, b1 = 0;
		in >> p1[i].X[0] >> p1[i].X[1] >> p1[i].X[2] >> b1 >> i2 >> p2[i].X[0] >> p2[i].X[1] >> p2[i].X[2] >> p2[i].bad;
		p1[i].bad = b1 == 1;
		kf[0].mvpMapPoints.push_back(b1 == 2 ? nullptr : &p1[i]);
		p2[i].kf = &kf[1]; p2[i].idx = i2;
		if (i2 > -2) vpMatches1[i] = &p2[i];
	}
	if (!in) { std::fprintf(stderr, "bad scene file\n"); return 3; }
	Context ctx(0);
	const int ret = cOptimizer::OptimizeSim3(ctx, &kf[0], &kf[1], vpMatches1, S);
	std::printf("%d\n", ret);
	for (double v : S.q) std::printf(" %a", v);
	for (double v : S.t) std::printf(" %a", v);
	std::printf(" %a", S.s);
	for (double v : S.R) std::printf(" %a", v);
	std::printf("\n");
	for (MapPoint* m : vpMatches1) std::printf("%d", m ? 1 : 0);
	std::printf("\n");
	return 0;
}
