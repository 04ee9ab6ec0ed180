// Driver for tests/test_gpu_kfdb_facade.py: MultiColSLAM::cMultiKeyFrameDatabase (include/mcs/mcs_facade.hpp) end to end.
// in:  nkf nq, per keyframe: id, nwords, words, values, ncovis, covis ids; per query: id, nwords, words, values
// out: per query the relocalisation candidates (batched), then the same queries one by one with new ids (id + 1000000),
//      then a loop query per keyframe 0..3 (minScore 0, connected = its covisibles), then score(query 0, all keyframes)
#include "mcs/mcs_facade.hpp"

struct KF {
	unsigned long mnId = 0;
	std::map<unsigned, double> mBowVec;
	std::vector<unsigned long> covis;
};

template <class T> static T rd(FILE* f) { T v{}; if (std::fread(&v, sizeof(T), 1, f) != 1) throw std::runtime_error("short input"); return v; }

static void readBow(FILE* f, KF& k) {
	k.mnId = (unsigned long)rd<int64_t>(f);
	const int n = rd<int32_t>(f);
	std::vector<int32_t> w(n);
	for (auto& x : w) x = rd<int32_t>(f);
	for (int i = 0; i < n; ++i) k.mBowVec[(unsigned)w[i]] = rd<double>(f);
}

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	try {
		FILE* fi = std::fopen(argv[1], "rb");
		if (!fi) return 2;
		const int nkf = rd<int32_t>(fi), nq = rd<int32_t>(fi), nWords = rd<int32_t>(fi);
		std::vector<KF> kfs(nkf), qs(nq);
		std::map<unsigned long, KF*> byId;
		for (auto& k : kfs) {
			readBow(fi, k);
			const int nc = rd<int32_t>(fi);
			for (int i = 0; i < nc; ++i) k.covis.push_back((unsigned long)rd<int64_t>(fi));
			byId[k.mnId] = &k;
		}
		for (auto& q : qs) readBow(fi, q);
		std::fclose(fi);
		MultiColSLAM::Context ctx(0);
		MultiColSLAM::cMultiKeyFrameDatabase<KF> db(ctx, nWords);
		for (auto& k : kfs) db.add(&k);
		for (auto& k : kfs) {
			std::vector<KF*> nb;
			for (unsigned long id : k.covis) nb.push_back(byId.at(id));
			db.SetCovisibility(&k, nb);
		}
		FILE* fo = std::fopen(argv[2], "wb");
		auto put = [&](const std::vector<KF*>& v) {
			const int32_t n = (int32_t)v.size();
			std::fwrite(&n, 4, 1, fo);
			for (KF* k : v) { const int64_t id = (int64_t)k->mnId; std::fwrite(&id, 8, 1, fo); }
		};
		std::vector<KF*> qp;
		for (auto& q : qs) qp.push_back(&q);
		for (auto& r : db.DetectRelocalisationCandidates(qp)) put(r);
		for (auto& q : qs) { q.mnId += 1000000; put(db.DetectRelocalisationCandidates(&q)); }
		for (int i = 0; i < 4 && i < nkf; ++i) {
			std::set<KF*> conn;
			for (unsigned long id : kfs[i].covis) conn.insert(byId.at(id));
			put(db.DetectLoopCandidates(&kfs[i], 0.0, conn));
		}
		std::vector<KF*> all;
		for (auto& k : kfs) all.push_back(&k);
		const std::vector<double> s = db.score(qs[0].mBowVec, all);
		std::fwrite(s.data(), 8, s.size(), fo);
		std::fclose(fo);
	} catch (const std::exception& e) {
		std::fprintf(stderr, "facade_driver_kfdb: %s\n", e.what());
		return 1;
	}
	return 0;
}
