// facade_driver_poseopt.cpp — MultiColSLAM::cOptimizer::PoseOptimization of include/mcs/mcs_facade.hpp on frames read from a text file, over a rig loaded by
// LoadMCS.  usage: facade_driver_poseopt <calibration dir> <scene file>.  Scene file: nframes; per frame: 6 pose numbers, huber, n, then n lines
// "x y octave cam point" (point -1 = NULL); then npoints and npoints lines "X Y Z"; then nlevels and the mvInvLevelSigma2 values.  Prints per frame (hex floats):
// the return value, `inliers`, the 6 pose numbers, the outlier flags, MtMc_inv of every camera; then the same frames through the batched call.
#include "mcs/mcs_facade.hpp"

#include <cstdio>
#include <fstream>
#include <map>

using namespace MultiColSLAM;

struct MapPoint {
	double X[3];
	bool bad = false;
	const double* GetWorldPos() const { return X; }
	bool isBad() const { return bad; }
};
struct Frame {
	cMultiCamSys_ camSystem;
	std::vector<KeyPoint> mvKeys;
	std::map<size_t, int> keypoint_to_cam;
	std::vector<MapPoint*> mvpMapPoints;
	std::vector<bool> mvbOutlier;
	std::vector<double> mvInvLevelSigma2;
	double huber = 1.0;
};

static void print(const Frame& F, int ret, double inliers) {
	std::printf("%d %a", ret, inliers);
	for (double v : F.camSystem.M_t_min) std::printf(" %a", v);
	std::printf("\n");
	for (bool o : F.mvbOutlier) std::printf("%d", o ? 1 : 0);
	std::printf("\n");
	for (const Matx44d& M : F.camSystem.MtMc_inv) for (double v : M) std::printf(" %a", v);
	std::printf("\n");
}

int main(int argc, char** argv) {
	if (argc != 3) { std::fprintf(stderr, "usage: %s <calibration dir> <scene file>\n", argv[0]); return 2; }
	cMultiCamSys_ rig;
	LoadMCS(argv[1], rig);
	std::ifstream in(argv[2]);
	size_t nframes = 0;
	in >> nframes;
	std::vector<Frame> frames(nframes);
	std::vector<std::vector<int>> ids(nframes);
	for (size_t f = 0; f < nframes; ++f) {
		Frame& F = frames[f];
		F.camSystem = rig;
		std::array<double, 6> pose;
		for (double& v : pose) in >> v;
		F.camSystem.Set_M_t_from_min(pose);
		size_t n = 0;
		in >> F.huber >> n;
		F.mvKeys.resize(n); F.mvbOutlier.assign(n, true); ids[f].resize(n);
		for (size_t i = 0; i < n; ++i) {
			KeyPoint& k = F.mvKeys[i];
			int cam = 0;
			k = KeyPoint{};
			in >> k.ptx >> k.pty >> k.octave >> cam >> ids[f][i];
			F.keypoint_to_cam[i] = cam;
		}
	}
	size_t npoints = 0;
	in >> npoints;
	std::vector<MapPoint> points(npoints);
	for (MapPoint& p : points) in >> p.X[0] >> p.X[1] >> p.X[2];
	size_t nlevels = 0;
	in >> nlevels;
	std::vector<double> sigma(nlevels);
	for (double& v : sigma) in >> v;
	if (!in) { std::fprintf(stderr, "bad scene file\n"); return 3; }
	for (size_t f = 0; f < nframes; ++f) {
		frames[f].mvInvLevelSigma2 = sigma;
		for (int id : ids[f]) frames[f].mvpMapPoints.push_back(id < 0 ? nullptr : &points[(size_t)id]);
	}
	Context ctx(0);
	std::vector<Frame> single = frames;
	for (Frame& F : single) {
		double inliers = -1.0;
		const int ret = cOptimizer::PoseOptimization(ctx, &F, inliers, F.huber);
		print(F, ret, inliers);
	}
	std::vector<Frame*> batch;
	std::vector<double> huber, share;
	for (Frame& F : frames) { batch.push_back(&F); huber.push_back(F.huber); }
	const std::vector<int> ret = cOptimizer::PoseOptimizationBatch<Frame, MapPoint>(ctx, batch, share, huber);
	for (size_t f = 0; f < nframes; ++f) print(frames[f], ret[f], share[f]);
	return 0;
}
