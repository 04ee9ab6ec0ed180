// facade_driver_essgraph.cpp — MultiColSLAM::cOptimizer::OptimizeEssentialGraph of include/mcs/mcs_facade.hpp on a little map read from a text file.
// usage: facade_driver_essgraph <scene file>.  Scene file: nk, then per keyframe (in the order GetAllKeyFrames() returns them) "mnId bad", the 16 numbers of
// GetPoseInverse() (row-major), the index of its parent or -1, nl and its loop edges as indices, nc and its covisible keyframes as indices in
// GetVectorCovisibleKeyFrames() order, nw and nw pairs "index weight" (GetWeight; 0 where none is given); the indices of pLoopMKF and pCurMKF; the number of
// CorrectedSim3 entries and per entry an index and eight numbers (qx qy qz qw tx ty tz s), the same for NonCorrectedSim3; the number of LoopConnections
// entries and per entry an index, a count and that many indices; np and np lines "X Y Z bad reference mnCorrectedByKF mnCorrectedReference" (reference: an
// index).  Prints (hex floats): the status, iterations, stop reason and the trials; per keyframe "set" (0 / 1) and the 16 numbers SetPose received; per point
// "X Y Z".
#include "mcs/mcs_facade.hpp"

#include <cstdio>
#include <fstream>
#include <map>
#include <set>

using namespace MultiColSLAM;

struct KeyFrame {
	long unsigned int mnId = 0;
	bool bad = false, set = false;
	Matx44d poseInv{}, pose{};
	KeyFrame* parent = nullptr;
	std::set<KeyFrame*> loops;
	std::vector<KeyFrame*> cov;
	std::map<KeyFrame*, int> weight;
	bool isBad() const { return bad; }
	Matx44d GetPoseInverse() const { return poseInv; }
	KeyFrame* GetParent() const { return parent; }
	std::set<KeyFrame*> GetLoopEdges() const { return loops; }
	int GetWeight(KeyFrame* k) const { const auto it = weight.find(k); return it == weight.end() ? 0 : it->second; }
	std::vector<KeyFrame*> GetCovisiblesByWeight(int w) const {
		std::vector<KeyFrame*> r;
		for (KeyFrame* k : cov) if (GetWeight(k) >= w) r.push_back(k);
		return r;
	}
	void SetPose(const Matx44d& M) { pose = M; set = true; }
};
struct MapPoint {
	double X[3] = {0, 0, 0};
	bool bad = false;
	KeyFrame* ref = nullptr;
	long mnCorrectedByKF = -1, mnCorrectedReference = -1;
	bool isBad() const { return bad; }
	const double* GetWorldPos() const { return X; }
	void SetWorldPos(const double* p) { X[0] = p[0]; X[1] = p[1]; X[2] = p[2]; }
	KeyFrame* GetReferenceKeyFrame() const { return ref; }
};
struct Map {
	std::vector<KeyFrame*> kfs;
	std::vector<MapPoint*> mps;
	std::vector<KeyFrame*> GetAllKeyFrames() const { return kfs; }
	std::vector<MapPoint*> GetAllMapPoints() const { return mps; }
};

int main(int argc, char** argv) {
	if (argc != 2) { std::fprintf(stderr, "usage: %s <scene file>\n", argv[0]); return 2; }
	std::ifstream in(argv[1]);
	size_t nk = 0;
	in >> nk;
	std::vector<KeyFrame> kf(nk);
	for (KeyFrame& k : kf) {
		long parent = -1;
		size_t n = 0;
		in >> k.mnId >> k.bad;
		for (double& v : k.poseInv) in >> v;
		in >> parent;
		if (parent >= 0) k.parent = &kf[(size_t)parent];
		in >> n;
		for (size_t i = 0; i < n; ++i) { size_t j = 0; in >> j; k.loops.insert(&kf[j]); }
		in >> n;
		for (size_t i = 0; i < n; ++i) { size_t j = 0; in >> j; k.cov.push_back(&kf[j]); }
		in >> n;
		for (size_t i = 0; i < n; ++i) { size_t j = 0; int w = 0; in >> j >> w; k.weight[&kf[j]] = w; }
	}
	size_t loop = 0, cur = 0, n = 0;
	in >> loop >> cur;
	std::map<KeyFrame*, cOptimizer::EgSim3> tables[2];
	for (auto& table : tables) {
		in >> n;
		for (size_t i = 0; i < n; ++i) {
			size_t j = 0;
			cOptimizer::EgSim3 S{};
			in >> j;
			for (double& v : S) in >> v;
			table[&kf[j]] = S;
		}
	}
	std::map<KeyFrame*, std::set<KeyFrame*>> conns;
	in >> n;
	for (size_t i = 0; i < n; ++i) {
		size_t j = 0, m = 0;
		in >> j >> m;
		for (size_t q = 0; q < m; ++q) { size_t c = 0; in >> c; conns[&kf[j]].insert(&kf[c]); }
	}
	size_t np = 0;
	in >> np;
	std::vector<MapPoint> pts(np);
	for (MapPoint& p : pts) {
		size_t r = 0;
		in >> p.X[0] >> p.X[1] >> p.X[2] >> p.bad >> r >> p.mnCorrectedByKF >> p.mnCorrectedReference;
		p.ref = &kf[r];
	}
	if (!in) { std::fprintf(stderr, "bad scene file\n"); return 3; }
	Map map;
	for (KeyFrame& k : kf) map.kfs.push_back(&k);
	for (MapPoint& p : pts) map.mps.push_back(&p);
	Context ctx(0);
	mcs_eg_diag d{};
	cOptimizer::EgSim3 Scurw{};
	const int status = cOptimizer::OptimizeEssentialGraph(ctx, &map, &kf[loop], &kf[cur], Scurw, tables[1], tables[0], conns, &d);
	std::printf("%d %d %d", status, d.iters, d.stop);
	for (int t : d.trials) std::printf(" %d", t);
	std::printf("\n");
	for (const KeyFrame& k : kf) {
		std::printf("%d", k.set ? 1 : 0);
		for (double v : k.pose) std::printf(" %a", v);
		std::printf("\n");
	}
	for (const MapPoint& p : pts) std::printf("%a %a %a\n", p.X[0], p.X[1], p.X[2]);
	return 0;
}
