// mcs_kfdb.hip — cMultiKeyFrameDatabase (src/cMultiKeyFrameDatabase.cpp) on the device, and the BowVector of one multi-frame from the leaf
// nodes of mcs_bow_transform (ThirdParty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1205, BowVector.cpp normalize).
//
// The inverted file is not kept as lists: a keyframe is a row of its BowVector (ascending word ids, L1-normalised doubles) in a growable slab,
// with a slot, its mnId, an add sequence number (re-set on re-add) and its persistent query state.  The list order of the reference
// (lKFsSharingWords: smallest word shared with the query, then position in that word's inverted list = add order) is the key
// (smallest shared word << 32 | add sequence).  A batch of queries runs as
//   k_qbitmap   word bitmap per query (+ validation of the query words)
//   k_count     shared-word count and smallest shared word per (query, slot): one wave per keyframe streams its word list past the bitmaps
//               of up to 16 queries (in LDS when they fit, else read from global memory: vocabularies of ~1 M words)
//   k_walk      one thread per slot walks the queries in batch order: the mnRelocQuery / mnRelocWords (mnLoopQuery / mnLoopWords) updates
//               of the word walk, exactly as the sequential calls would leave them (traps (b), (c) of DESIGN §7)
//   k_maxc      maxCommonWords / minCommonWords per query
//   k_score     DBoW2 L1Scoring::score of every candidate above minCommonWords, one thread per pair, left to right in ascending word order
//   k_carry     one thread per slot: the score a neighbour shows in query q (this query's, else the latest earlier one's, else the
//               persistent one — trap (a))
//   k_final     one workgroup per query: covisibility accumulation, list order, 0.75 * bestAccScore retention, dedup, outputs
// The new persistent state is written to the second copy of the state arrays and becomes current only when the whole call succeeds.
#include "mcs_host.h"
#include <unordered_map>

namespace mcs {

constexpr int KF_COVIS = 10;   // GetBestCovisibilityKeyFrames(10)
constexpr int KF_QG = 16;      // queries per k_count workgroup
constexpr int KF_LDS_BYTES = 48 * 1024;
enum { F_APPENDED = 1, F_QMATCH = 2, F_SCORED = 4, F_INLIST = 8 };

// DBoW2 L1Scoring::score (ThirdParty/DBoW2/DBoW2/ScoringObject.cpp:23-66): shared words in ascending id order, vi from the FIRST vector
__device__ double l1_score(const int* aw, const double* av, int na, const int* bw, const double* bv, int nb) {
	double score = 0;
	int i = 0, j = 0;
	while (i < na && j < nb) {
		const int x = aw[i], y = bw[j];
		if (x == y) {
			const double vi = av[i], wi = bv[j];
			score += fabs(vi - wi) - fabs(vi) - fabs(wi);
			++i; ++j;
		} else if (x < y) {
			++i;
		} else {
			++j;
		}
	}
	return -score / 2.0;
}

// bits of every query's words; err[0] |= 1 for a word out of range, 2 for a row that is not strictly ascending
__global__ __launch_bounds__(256) void k_qbitmap(const int* qOff, const int* qWords, int nq, int nWords, int bmWords, uint32_t* bm, int* err) {
	const int q = blockIdx.x;
	if (q >= nq) return;
	const int lo = qOff[q], hi = qOff[q + 1];
	for (int k = lo + threadIdx.x; k < hi; k += 256) {
		const int w = qWords[k];
		if (w < 0 || w >= nWords) { atomicOr(err, 1); continue; }
		if (k > lo && qWords[k - 1] >= w) atomicOr(err, 2);
		atomicOr(&bm[(size_t)q * bmWords + (w >> 5)], 1u << (w & 31));
	}
}

struct CountArgs {
	const uint32_t* bm; int bmWords; int nq; int S;
	const int* rowOff; const int* rowLen; const int* active; const int* words;
	int* cnt; int* minw;
};

template <bool kLds>
__global__ __launch_bounds__(256) void k_count(CountArgs a) {
	extern __shared__ uint32_t sbm[];
	const int q0 = blockIdx.y * KF_QG;
	const int nqg = min(KF_QG, a.nq - q0);
	const uint32_t* bm = a.bm + (size_t)q0 * a.bmWords;
	if (kLds) {
		for (int i = threadIdx.x; i < nqg * a.bmWords; i += 256) sbm[i] = bm[i];
		__syncthreads();
		bm = sbm;
	}
	const int lane = threadIdx.x & 63;
	const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (s >= a.S) return;
	int cnt[KF_QG], mn[KF_QG];
#pragma unroll
	for (int i = 0; i < KF_QG; ++i) { cnt[i] = 0; mn[i] = 0x7FFFFFFF; }
	if (a.active[s]) {
		const int* row = a.words + a.rowOff[s];
		const int n = a.rowLen[s];
		for (int k = lane; k < n; k += 64) {
			const int w = row[k];
			const int wi = w >> 5;
			const uint32_t bit = 1u << (w & 31);
#pragma unroll
			for (int i = 0; i < KF_QG; ++i) {
				if (i < nqg && (bm[(size_t)i * a.bmWords + wi] & bit)) {
					++cnt[i];
					mn[i] = min(mn[i], w);
				}
			}
		}
	}
#pragma unroll
	for (int i = 0; i < KF_QG; ++i) {
		int c = cnt[i], m = mn[i];
		for (int o = 32; o > 0; o >>= 1) {
			c += __shfl_xor(c, o);
			m = min(m, __shfl_xor(m, o));
		}
		if (lane == 0 && i < nqg) {
			a.cnt[(size_t)(q0 + i) * a.S + s] = c;
			a.minw[(size_t)(q0 + i) * a.S + s] = m;
		}
	}
}

// the word walk of every query in batch order, per slot (src/cMultiKeyFrameDatabase.cpp:94-113 loop, :226-241 relocalisation)
struct WalkArgs {
	int nq; int S; int loop;
	const int64_t* qid; const uint8_t* conn;   // conn[q*S + s]: slot s is in query q's connected set (loop form)
	const int* cnt;
	const int64_t* curQ; const int* curW;
	int64_t* nextQ; int* nextW;
	int* wordsAfter; uint8_t* flags;
};

__global__ __launch_bounds__(256) void k_walk(WalkArgs a) {
	const int s = blockIdx.x * 256 + threadIdx.x;
	if (s >= a.S) return;
	int64_t Q = a.curQ[s];
	int W = a.curW[s];
	for (int q = 0; q < a.nq; ++q) {
		const size_t o = (size_t)q * a.S + s;
		const int c = a.cnt[o];
		const int64_t id = a.qid[q];
		uint8_t f = 0;
		if (c > 0) {
			if (Q != id) {
				if (a.loop && a.conn[o]) {
					W = 1;   // reset to 0 on every visit, mnLoopQuery never set: 1 after the last visit
				} else {
					W = c;
					Q = id;
					f |= F_APPENDED;
				}
			} else {
				W += c;   // stored query id already equal: counting continues, never appended (trap (b))
			}
		}
		if (Q == id) f |= F_QMATCH;
		a.wordsAfter[o] = W;
		a.flags[o] = f;
	}
	a.nextQ[s] = Q;
	a.nextW[s] = W;
}

// maxCommonWords over the appended keyframes; minCommonWords = static_cast<int>(maxCommonWords * 0.8)
__global__ __launch_bounds__(256) void k_maxc(int S, const int* wordsAfter, const uint8_t* flags, int* minC, int* nApp) {
	const int q = blockIdx.x;
	__shared__ int smax[256], sn[256];
	int mx = 0, n = 0;
	for (int s = threadIdx.x; s < S; s += 256) {
		const size_t o = (size_t)q * S + s;
		if (flags[o] & F_APPENDED) { mx = max(mx, wordsAfter[o]); ++n; }
	}
	smax[threadIdx.x] = mx; sn[threadIdx.x] = n;
	__syncthreads();
	for (int st = 128; st > 0; st >>= 1) {
		if (threadIdx.x < st) { smax[threadIdx.x] = max(smax[threadIdx.x], smax[threadIdx.x + st]); sn[threadIdx.x] += sn[threadIdx.x + st]; }
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		minC[q] = static_cast<int>((double)smax[0] * 0.8);
		nApp[q] = sn[0];
	}
}

struct ScoreArgs {
	int nq; int S; int loop;
	const int* qOff; const int* qWords; const double* qVals; const double* minScore;
	const int* rowOff; const int* rowLen; const int* words; const double* vals;
	const int* wordsAfter; const int* minC;
	uint8_t* flags; double* score;
};

__global__ __launch_bounds__(256) void k_score(ScoreArgs a) {
	const int s = blockIdx.x * 256 + threadIdx.x;
	const int q = blockIdx.y;
	if (s >= a.S) return;
	const size_t o = (size_t)q * a.S + s;
	uint8_t f = a.flags[o];
	if (!(f & F_APPENDED) || a.wordsAfter[o] <= a.minC[q]) return;
	const int lo = a.qOff[q];
	const double si = l1_score(a.qWords + lo, a.qVals + lo, a.qOff[q + 1] - lo, a.words + a.rowOff[s], a.vals + a.rowOff[s], a.rowLen[s]);
	f |= F_SCORED;
	if (!a.loop || si >= a.minScore[q]) f |= F_INLIST;
	a.flags[o] = f;
	a.score[o] = si;
}

// score[q*S + s] becomes the value mRelocScore / mLoopScore of slot s holds after query q's scoring step
__global__ __launch_bounds__(256) void k_carry(int nq, int S, const uint8_t* flags, double* score, const double* curS, double* nextS) {
	const int s = blockIdx.x * 256 + threadIdx.x;
	if (s >= S) return;
	double v = curS[s];
	for (int q = 0; q < nq; ++q) {
		const size_t o = (size_t)q * S + s;
		if (flags[o] & F_SCORED) v = score[o];
		else score[o] = v;
	}
	nextS[s] = v;
}

struct FinalArgs {
	int nq; int S; int loop;
	const double* minScore; const int* minC; const int* nApp;
	const int* wordsAfter; const uint8_t* flags; const double* score; const int* minw;
	const uint32_t* addSeq; const int64_t* slotId; const int* covis; const int* covisN;
	int* lSlot; uint64_t* lKey; double* lAcc; int* lBest; int* lOrder; uint8_t* seen;
	int cap; int64_t* candIds; int* candCount;
	int dcap; int* dCount; int64_t* dId; int* dWords; double* dScore; double* dAcc; int64_t* dBest;
};

__global__ __launch_bounds__(1024) void k_final(FinalArgs a) {
	const int q = blockIdx.x;
	const size_t base = (size_t)q * a.S;
	__shared__ int sn;
	__shared__ double sred[1024];
	if (threadIdx.x == 0) sn = 0;
	__syncthreads();
	if (a.nApp[q] > 0) {
		for (int s = threadIdx.x; s < a.S; s += 1024)
			if (a.flags[base + s] & F_INLIST) a.lSlot[base + atomicAdd(&sn, 1)] = s;
	}
	__syncthreads();
	const int n = sn;
	const int minC = a.minC[q];
	// covisibility accumulation per list entry (:150-170 loop, :283-305 relocalisation); the order across entries does not matter here
	for (int i = threadIdx.x; i < n; i += 1024) {
		const int s = a.lSlot[base + i];
		const double si = a.score[base + s];
		double bestScore = si, acc = si;
		int best = s;
		const int nn = a.covisN[s];
		for (int k = 0; k < nn; ++k) {
			const int nb = a.covis[(size_t)s * KF_COVIS + k];
			const size_t ob = base + nb;
			if (!(a.flags[ob] & F_QMATCH)) continue;
			if (a.loop && a.wordsAfter[ob] <= minC) continue;
			const double v = a.score[ob];
			acc += v;
			if (v > bestScore) { best = nb; bestScore = v; }
		}
		a.lAcc[base + i] = acc;
		a.lBest[base + i] = best;
		a.lKey[base + i] = ((uint64_t)(uint32_t)a.minw[base + s] << 32) | a.addSeq[s];
	}
	__syncthreads();
	// list order: rank by (smallest shared word, add sequence); the keys are distinct
	double mx = a.loop ? a.minScore[q] : 0.0;
	for (int i = threadIdx.x; i < n; i += 1024) {
		const uint64_t key = a.lKey[base + i];
		int r = 0;
		for (int j = 0; j < n; ++j) r += a.lKey[base + j] < key;
		a.lOrder[base + r] = i;
		const double v = a.lAcc[base + i];
		if (v > mx) mx = v;
	}
	sred[threadIdx.x] = mx;
	__syncthreads();
	for (int st = 512; st > 0; st >>= 1) {
		if (threadIdx.x < st && sred[threadIdx.x + st] > sred[threadIdx.x]) sred[threadIdx.x] = sred[threadIdx.x + st];
		__syncthreads();
	}
	if (threadIdx.x != 0) return;
	const double minScoreToRetain = 0.75 * sred[0];
	int nc = 0;
	for (int r = 0; r < n; ++r) {
		const int i = a.lOrder[base + r];
		const int s = a.lSlot[base + i];
		const double acc = a.lAcc[base + i];
		const int b = a.lBest[base + i];
		if (r < a.dcap) {
			const size_t d = (size_t)q * a.dcap + r;
			a.dId[d] = a.slotId[s]; a.dWords[d] = a.wordsAfter[base + s]; a.dScore[d] = a.score[base + s]; a.dAcc[d] = acc; a.dBest[d] = a.slotId[b];
		}
		if (acc > minScoreToRetain && !a.seen[base + b]) {
			a.seen[base + b] = 1;
			if (nc < a.cap) a.candIds[(size_t)q * a.cap + nc] = a.slotId[b];
			++nc;
		}
	}
	a.candCount[q] = nc;
	a.dCount[q] = n;
}

// ORBVocabulary::score(query, keyframe) for a list of stored keyframes
__global__ __launch_bounds__(256) void k_score_list(const int* qw, const double* qv, int nqw, const int* slots, int n, const int* rowOff, const int* rowLen,
                                                    const int* words, const double* vals, double* out) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int s = slots[i];
	out[i] = l1_score(qw, qv, nqw, words + rowOff[s], vals + rowOff[s], rowLen[s]);
}

// BowVector of one frame from its leaf nodes (TemplatedVocabulary::transform, TF_IDF branch :1147-1163, then BowVector::normalize(L1)).
// Every addend of a word is that word's one weight, so the value is `count` sequential additions of it; no sort of the features is needed.
// hist (n_words ints) is zero between calls: the kernel clears what it touched.
__global__ __launch_bounds__(1024) void k_bow_vector(const int* leaf, int n, int nNodes, int nWords, const int* wordOf, const double* weightOf, int* hist, int* dW,
                                                     double* dWt, int* outW, double* outV, int* nOut, int* err) {
	__shared__ int sd;
	__shared__ double snorm;
	if (threadIdx.x == 0) sd = 0;
	__syncthreads();
	for (int i = threadIdx.x; i < n; i += 1024) {
		const int nd = leaf[i];
		if (nd < 0 || nd >= nNodes) { atomicOr(err, 1); continue; }
		const double w = weightOf[nd];
		if (!(w > 0)) continue;
		const int wid = wordOf[nd];
		if (wid < 0 || wid >= nWords) { atomicOr(err, 2); continue; }
		if (atomicAdd(&hist[wid], 1) == 0) {
			const int k = atomicAdd(&sd, 1);
			dW[k] = wid; dWt[k] = w;
		}
	}
	__syncthreads();
	const int d = sd;
	for (int k = threadIdx.x; k < d; k += 1024) {
		const int wid = dW[k];
		int r = 0;
		for (int j = 0; j < d; ++j) r += dW[j] < wid;
		const double w = dWt[k];
		double v = w;
		for (int c = hist[wid]; c > 1; --c) v += w;
		outW[r] = wid;
		outV[r] = v;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		double norm = 0.0;
		for (int r = 0; r < d; ++r) norm += fabs(outV[r]);
		snorm = norm;
		*nOut = d;
	}
	__syncthreads();
	const double norm = snorm;
	for (int k = threadIdx.x; k < d; k += 1024) {
		if (norm > 0.0) outV[k] /= norm;
		hist[dW[k]] = 0;
	}
}

}  // namespace mcs

using namespace mcs;

// ------------------------------------------------------------------ vocabulary words (the node table of TemplatedVocabulary: m_nodes[i].word_id / weight)

struct mcs_vocabulary;
int mcs_vocabulary_words_internal(mcs_vocabulary* v, mcs_ctx** c, int* nNodes, int** wordOf, double** weightOf, int** hist, int* nWords);
int mcs_vocabulary_set_words_internal(mcs_vocabulary* v, const int32_t* word_id_per_node, const double* weight_per_node);

namespace {

template <class T>
hipError_t grow(T** p, size_t& cap, size_t need, size_t keep) {
	if (need <= cap) return hipSuccess;
	size_t nc = std::max<size_t>(need, cap * 2);
	nc = std::max<size_t>(nc, 64);
	T* np = nullptr;
	hipError_t e = hipMalloc((void**)&np, nc * sizeof(T));
	if (e != hipSuccess) return e;
	if (*p && keep) e = hipMemcpy(np, *p, keep * sizeof(T), hipMemcpyDeviceToDevice);
	if (*p) (void)hipFree(*p);
	*p = np;
	cap = nc;
	return e;
}

// copy `bytes` of a caller array (host or device) into a host vector
template <class T>
hipError_t fetch(std::vector<T>& dst, const T* src, size_t n, mcs_mem_kind kind) {
	dst.resize(n);
	if (!n) return hipSuccess;
	if (kind == MCS_MEM_HOST) { memcpy(dst.data(), src, n * sizeof(T)); return hipSuccess; }
	return hipMemcpy(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost);
}

}  // namespace

struct mcs_kfdb {
	mcs_ctx* ctx = nullptr;
	int nWords = 0, bmWords = 0;
	// slots: every keyframe id the database has seen (added, erased, or named as a covisible neighbour) keeps one, with its state
	std::unordered_map<int64_t, int> slotOf;
	std::vector<int64_t> id;
	std::vector<int> rowOff, rowLen, active, covisN, covis;
	std::vector<uint32_t> addSeq;
	uint32_t seq = 0;
	bool metaDirty = true;
	size_t slabUsed = 0, slabCap = 0, slabValsCap = 0;
	int* words = nullptr; double* vals = nullptr;
	// device copies of the slot metadata
	size_t slotCap = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0;
	int* dRowOff = nullptr; int* dRowLen = nullptr; int* dActive = nullptr; int* dCovisN = nullptr; int* dCovis = nullptr; uint32_t* dAddSeq = nullptr;
	int64_t* dId = nullptr;
	// persistent state, two copies each (current / next): [0] relocalisation, [1] loop
	int cur[2] = {0, 0};
	int64_t* stQ[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
	int* stW[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
	double* stS[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
	size_t stCap = 0;
	// scratch of one batch
	DevBuf scratch;
};

static int kfdb_slot(mcs_kfdb* db, int64_t kid) {
	auto it = db->slotOf.find(kid);
	if (it != db->slotOf.end()) return it->second;
	const int s = (int)db->id.size();
	db->slotOf[kid] = s;
	db->id.push_back(kid);
	db->rowOff.push_back(0); db->rowLen.push_back(0); db->active.push_back(0); db->covisN.push_back(0);
	for (int k = 0; k < KF_COVIS; ++k) db->covis.push_back(0);
	db->addSeq.push_back(0);
	db->metaDirty = true;
	return s;
}

// device metadata and state arrays sized for every slot; new slots get the state of a keyframe never queried (query ids 0, counters 0, scores 0.0)
static int kfdb_sync(mcs_kfdb* db) {
	const size_t S = db->id.size();
	if (S > db->stCap) {
		const size_t nc = std::max<size_t>(S * 2, 256);
		for (int m = 0; m < 2; ++m)
			for (int b = 0; b < 2; ++b) {
				int64_t* q = nullptr; int* w = nullptr; double* s = nullptr;
				HIPCHK(hipMalloc((void**)&q, nc * 8)); HIPCHK(hipMalloc((void**)&w, nc * 4)); HIPCHK(hipMalloc((void**)&s, nc * 8));
				HIPCHK(hipMemset(q, 0, nc * 8)); HIPCHK(hipMemset(w, 0, nc * 4)); HIPCHK(hipMemset(s, 0, nc * 8));
				if (db->stQ[m][b] && db->stCap) {
					HIPCHK(hipMemcpy(q, db->stQ[m][b], db->stCap * 8, hipMemcpyDeviceToDevice));
					HIPCHK(hipMemcpy(w, db->stW[m][b], db->stCap * 4, hipMemcpyDeviceToDevice));
					HIPCHK(hipMemcpy(s, db->stS[m][b], db->stCap * 8, hipMemcpyDeviceToDevice));
				}
				(void)hipFree(db->stQ[m][b]); (void)hipFree(db->stW[m][b]); (void)hipFree(db->stS[m][b]);
				db->stQ[m][b] = q; db->stW[m][b] = w; db->stS[m][b] = s;
			}
		db->stCap = nc;
	}
	if (!db->metaDirty) return MCS_OK;
	HIPCHK(grow(&db->dRowOff, db->c1, S, 0)); HIPCHK(grow(&db->dRowLen, db->c2, S, 0)); HIPCHK(grow(&db->dActive, db->c3, S, 0));
	HIPCHK(grow(&db->dCovisN, db->c4, S, 0)); HIPCHK(grow(&db->dCovis, db->c5, S * KF_COVIS, 0)); HIPCHK(grow(&db->dAddSeq, db->slotCap, S, 0));
	HIPCHK(grow(&db->dId, db->c6, S, 0));
	if (S) {
		HIPCHK(hipMemcpy(db->dRowOff, db->rowOff.data(), S * 4, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(db->dRowLen, db->rowLen.data(), S * 4, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(db->dActive, db->active.data(), S * 4, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(db->dCovisN, db->covisN.data(), S * 4, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(db->dCovis, db->covis.data(), S * KF_COVIS * 4, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(db->dAddSeq, db->addSeq.data(), S * 4, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(db->dId, db->id.data(), S * 8, hipMemcpyHostToDevice));
	}
	db->metaDirty = false;
	return MCS_OK;
}

int mcs_kfdb_create(mcs_ctx* c, int n_words, int capacity_hint, mcs_kfdb** out) {
	if (!c || !out) return fail(MCS_ERR_INVALID, "null argument");
	if (n_words < 1) return fail(MCS_ERR_INVALID, "n_words must be >= 1");
	HIPCHK(hipSetDevice(c->device));
	mcs_kfdb* db = new mcs_kfdb();
	db->ctx = c; db->nWords = n_words; db->bmWords = (n_words + 31) / 32;
	if (capacity_hint > 0) {
		db->id.reserve(capacity_hint);
		const hipError_t e = grow(&db->words, db->slabCap, (size_t)capacity_hint * 1024, 0);
		const hipError_t e2 = e == hipSuccess ? grow(&db->vals, db->slabValsCap, (size_t)capacity_hint * 1024, 0) : e;
		if (e2 != hipSuccess) { mcs_kfdb_destroy(db); return fail(MCS_ERR_HIP, "keyframe database allocation failed"); }
	}
	*out = db;
	return MCS_OK;
}

int mcs_kfdb_destroy(mcs_kfdb* db) {
	if (!db) return MCS_OK;
	(void)hipSetDevice(db->ctx->device);
	(void)hipFree(db->words); (void)hipFree(db->vals);
	(void)hipFree(db->dRowOff); (void)hipFree(db->dRowLen); (void)hipFree(db->dActive); (void)hipFree(db->dCovisN); (void)hipFree(db->dCovis);
	(void)hipFree(db->dAddSeq); (void)hipFree(db->dId);
	for (int m = 0; m < 2; ++m)
		for (int b = 0; b < 2; ++b) { (void)hipFree(db->stQ[m][b]); (void)hipFree(db->stW[m][b]); (void)hipFree(db->stS[m][b]); }
	delete db;
	return MCS_OK;
}

int mcs_kfdb_clear(mcs_kfdb* db) {
	if (!db) return fail(MCS_ERR_INVALID, "null argument");
	for (size_t s = 0; s < db->id.size(); ++s) { db->active[s] = 0; db->rowLen[s] = 0; }
	db->slabUsed = 0;
	db->metaDirty = true;
	return MCS_OK;
}

int mcs_kfdb_size(const mcs_kfdb* db, int* n) {
	if (!db || !n) return fail(MCS_ERR_INVALID, "null argument");
	int k = 0;
	for (int a : db->active) k += a != 0;
	*n = k;
	return MCS_OK;
}

int mcs_kfdb_add(mcs_kfdb* db, int nkf, const int64_t* kf_ids, const int32_t* offsets, const int32_t* word_ids, const double* values, mcs_mem_kind kind) {
	if (!db || nkf < 0 || (nkf && (!kf_ids || !offsets))) return fail(MCS_ERR_INVALID, "null argument");
	if (nkf == 0) return MCS_OK;
	HIPCHK(hipSetDevice(db->ctx->device));
	std::vector<int64_t> ids;
	std::vector<int> off, w;
	HIPCHK(fetch(ids, kf_ids, nkf, kind));
	HIPCHK(fetch(off, offsets, (size_t)nkf + 1, kind));
	if (int r = guard_bow_offsets(off.data(), nkf, "mcs_kfdb_add")) return r;   // before anything is sized by them
	const size_t total = (size_t)off[nkf];
	if (total && (!word_ids || !values)) return fail(MCS_ERR_INVALID, "null word / value array");
	HIPCHK(fetch(w, word_ids, total, kind));
	if (int r = guard_bow_words(off.data(), nkf, w.data(), db->nWords, "mcs_kfdb_add")) return r;
	for (int i = 0; i < nkf; ++i) {
		auto it = db->slotOf.find(ids[i]);
		if (it != db->slotOf.end() && db->active[it->second])
			return fail(MCS_ERR_INVALID, "mcs_kfdb_add: keyframe " + std::to_string((long long)ids[i]) + " is already in the database");
		for (int j = 0; j < i; ++j)
			if (ids[j] == ids[i]) return fail(MCS_ERR_INVALID, "mcs_kfdb_add: keyframe " + std::to_string((long long)ids[i]) + " appears twice in one call");
	}
	if (db->seq + (uint64_t)nkf >= 0xFFFFFFFFull) return fail(MCS_ERR_CAPACITY, "mcs_kfdb_add: add sequence exhausted (clear the database)");
	const size_t base = db->slabUsed;
	HIPCHK(grow(&db->words, db->slabCap, base + total, base));
	HIPCHK(grow(&db->vals, db->slabValsCap, base + total, base));
	const hipMemcpyKind mk = kind == MCS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
	if (total) {
		HIPCHK(hipMemcpy(db->words + base, w.data(), total * 4, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(db->vals + base, values, total * 8, mk));
	}
	db->slabUsed = base + total;
	for (int i = 0; i < nkf; ++i) {
		const int s = kfdb_slot(db, ids[i]);
		db->rowOff[s] = (int)(base + off[i]);
		db->rowLen[s] = off[i + 1] - off[i];
		db->active[s] = 1;
		db->addSeq[s] = db->seq++;   // a re-added keyframe goes to the END of every inverted list (list::push_back)
	}
	db->metaDirty = true;
	return MCS_OK;
}

int mcs_kfdb_erase(mcs_kfdb* db, int nkf, const int64_t* kf_ids) {
	if (!db || nkf < 0 || (nkf && !kf_ids)) return fail(MCS_ERR_INVALID, "null argument");
	for (int i = 0; i < nkf; ++i) {
		auto it = db->slotOf.find(kf_ids[i]);
		if (it == db->slotOf.end() || !db->active[it->second]) continue;   // the reference's erase of an absent keyframe finds nothing to remove
		db->active[it->second] = 0;
		db->metaDirty = true;
	}
	return MCS_OK;
}

int mcs_kfdb_set_covisibility(mcs_kfdb* db, int nkf, const int64_t* kf_ids, const int64_t* neighbours, const int32_t* counts) {
	if (!db || nkf < 0 || (nkf && (!kf_ids || !neighbours || !counts))) return fail(MCS_ERR_INVALID, "null argument");
	for (int i = 0; i < nkf; ++i)
		if (counts[i] < 0 || counts[i] > KF_COVIS) return fail(MCS_ERR_INVALID, "covisibility counts must be in 0..10 (GetBestCovisibilityKeyFrames(10))");
	for (int i = 0; i < nkf; ++i) {
		const int s = kfdb_slot(db, kf_ids[i]);
		db->covisN[s] = counts[i];
		for (int k = 0; k < counts[i]; ++k) {
			const int nb = kfdb_slot(db, neighbours[(size_t)i * KF_COVIS + k]);
			db->covis[(size_t)s * KF_COVIS + k] = nb;
		}
	}
	db->metaDirty = true;
	return MCS_OK;
}

static int kfdb_detect(mcs_kfdb* db, int loop, int nq, const int64_t* query_ids, const int32_t* offsets, const int32_t* word_ids, const double* values,
                       const int32_t* conn_offsets, const int64_t* conn_ids, const double* min_scores, mcs_mem_kind kind, int cap, int32_t* cand_count,
                       int64_t* cand_ids, const mcs_kfdb_diag* diag) {
	if (!db || nq < 0 || (nq && (!query_ids || !offsets || !cand_count))) return fail(MCS_ERR_INVALID, "null argument");
	if (cap < 0 || (cap > 0 && !cand_ids)) return fail(MCS_ERR_INVALID, "cand_ids must hold nq * cap ids");
	if (loop && nq && !min_scores) return fail(MCS_ERR_INVALID, "null min_scores");
	if (diag && diag->cap > 0 && (!diag->count || !diag->kf_id || !diag->words || !diag->score || !diag->acc || !diag->best))
		return fail(MCS_ERR_INVALID, "diagnostics: null array");
	if (nq == 0) return MCS_OK;
	mcs_ctx* c = db->ctx;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	const bool host = kind == MCS_MEM_HOST;
	std::vector<int> off;
	HIPCHK(fetch(off, offsets, (size_t)nq + 1, kind));
	if (int r = guard_bow_offsets(off.data(), nq, nullptr)) return r;
	const size_t total = (size_t)off[nq];
	if (total && (!word_ids || !values)) return fail(MCS_ERR_INVALID, "null word / value array");
	std::vector<int64_t> qid;
	HIPCHK(fetch(qid, query_ids, nq, kind));
	if (host)
		if (int r = guard_bow_words(off.data(), nq, word_ids, db->nWords, loop ? "mcs_kfdb_detect_loop" : "mcs_kfdb_detect_relocalisation")) return r;
	int rc = kfdb_sync(db);
	if (rc != MCS_OK) return rc;
	const int S = (int)db->id.size();
	std::vector<uint8_t> conn;
	if (loop && conn_offsets) {
		std::vector<int> coff;
		std::vector<int64_t> cids;
		HIPCHK(fetch(coff, conn_offsets, (size_t)nq + 1, kind));
		if (coff[0] != 0) return fail(MCS_ERR_INVALID, "connected offsets[0] must be 0");
		for (int q = 0; q < nq; ++q)
			if (coff[q + 1] < coff[q]) return fail(MCS_ERR_INVALID, "connected offsets must be non-decreasing");
		if (coff[nq] && !conn_ids) return fail(MCS_ERR_INVALID, "null connected ids");
		HIPCHK(fetch(cids, conn_ids, (size_t)coff[nq], kind));
		conn.assign((size_t)nq * std::max(S, 1), 0);
		for (int q = 0; q < nq; ++q)
			for (int k = coff[q]; k < coff[q + 1]; ++k) {
				auto it = db->slotOf.find(cids[k]);
				if (it != db->slotOf.end()) conn[(size_t)q * S + it->second] = 1;
			}
	}
	if (S == 0) {   // empty database: nothing shares a word
		std::vector<int> z(nq, 0);
		if (host) memcpy(cand_count, z.data(), nq * 4); else HIPCHK(hipMemcpy(cand_count, z.data(), nq * 4, hipMemcpyHostToDevice));
		if (diag && diag->count) { if (host) memcpy(diag->count, z.data(), nq * 4); else HIPCHK(hipMemcpy(diag->count, z.data(), nq * 4, hipMemcpyHostToDevice)); }
		return MCS_OK;
	}
	const int dcap = diag ? std::max(diag->cap, 0) : 0;
	const size_t NS = (size_t)nq * S;
	// scratch layout
	uint32_t* bm = nullptr; int* err = nullptr; int* qOff = nullptr; int64_t* xQId = nullptr; double* xMinS = nullptr; int* xMinC = nullptr; int* xNApp = nullptr;
	int* xCnt = nullptr; int* xMinw = nullptr; int* xWA = nullptr; uint8_t* xFl = nullptr; double* xSc = nullptr; uint8_t* xConn = nullptr; int* xLSlot = nullptr;
	uint64_t* xLKey = nullptr; double* xLAcc = nullptr; int* xLBest = nullptr; int* xLOrd = nullptr; uint8_t* xSeen = nullptr; int* xCandN = nullptr;
	int64_t* xCand = nullptr; int* xDN = nullptr; int64_t* xDId = nullptr; int* xDW = nullptr; double* xDS = nullptr; double* xDA = nullptr; int64_t* xDB = nullptr;
	int* xQW = nullptr; double* xQV = nullptr;
	const size_t QC = (size_t)nq * std::max(cap, 1), QD = (size_t)nq * std::max(dcap, 1);
	Layout lay;
	lay.piece(&bm, (size_t)nq * db->bmWords * 4); lay.piece(&err, 4); lay.piece(&qOff, ((size_t)nq + 1) * 4); lay.piece(&xQId, (size_t)nq * 8);
	lay.piece(&xMinS, (size_t)nq * 8); lay.piece(&xMinC, (size_t)nq * 4); lay.piece(&xNApp, (size_t)nq * 4); lay.piece(&xCnt, NS * 4); lay.piece(&xMinw, NS * 4);
	lay.piece(&xWA, NS * 4); lay.piece(&xFl, NS); lay.piece(&xSc, NS * 8); lay.piece(&xConn, loop ? NS : 1); lay.piece(&xLSlot, NS * 4); lay.piece(&xLKey, NS * 8);
	lay.piece(&xLAcc, NS * 8); lay.piece(&xLBest, NS * 4); lay.piece(&xLOrd, NS * 4); lay.piece(&xSeen, NS); lay.piece(&xCandN, (size_t)nq * 4);
	lay.piece(&xCand, QC * 8); lay.piece(&xDN, (size_t)nq * 4); lay.piece(&xDId, QD * 8); lay.piece(&xDW, QD * 4); lay.piece(&xDS, QD * 8); lay.piece(&xDA, QD * 8);
	lay.piece(&xDB, QD * 8); lay.piece(&xQW, host ? total * 4 : 8); lay.piece(&xQV, host ? total * 8 : 8);
	HIPCHK(db->scratch.reserve(lay.total));
	lay.place(db->scratch.p);
	const int* dQWords = host ? xQW : word_ids;
	const double* dQVals = host ? xQV : values;
	HIPCHK(hipMemcpyAsync(qOff, off.data(), ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(xQId, qid.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
	if (loop) {
		std::vector<double> ms;
		HIPCHK(fetch(ms, min_scores, nq, kind));
		HIPCHK(hipMemcpyAsync(xMinS, ms.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
		if (conn.empty()) HIPCHK(hipMemsetAsync(xConn, 0, NS, st));
		else HIPCHK(hipMemcpyAsync(xConn, conn.data(), NS, hipMemcpyHostToDevice, st));
	}
	if (host && total) {
		HIPCHK(hipMemcpyAsync(xQW, word_ids, total * 4, hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(xQV, values, total * 8, hipMemcpyHostToDevice, st));
	}
	HIPCHK(hipMemsetAsync(bm, 0, (size_t)nq * db->bmWords * 4, st));
	HIPCHK(hipMemsetAsync(err, 0, 4, st));
	HIPCHK(hipMemsetAsync(xSeen, 0, NS, st));
	hipLaunchKernelGGL(k_qbitmap, dim3(nq), dim3(256), 0, st, (const int*)qOff, dQWords, nq, db->nWords, db->bmWords, bm, err);
	CountArgs ca{bm, db->bmWords, nq, S, db->dRowOff, db->dRowLen, db->dActive, db->words, xCnt, xMinw};
	const size_t ldsBytes = (size_t)KF_QG * db->bmWords * 4;
	const dim3 gc((S + 3) / 4, (nq + KF_QG - 1) / KF_QG);
	if (ldsBytes <= (size_t)KF_LDS_BYTES) hipLaunchKernelGGL(k_count<true>, gc, dim3(256), ldsBytes, st, ca);
	else hipLaunchKernelGGL(k_count<false>, gc, dim3(256), 0, st, ca);
	const int m = loop ? 1 : 0;
	const int cu = db->cur[m], nx = 1 - cu;
	WalkArgs wa{nq, S, loop, xQId, xConn, xCnt, db->stQ[m][cu], db->stW[m][cu], db->stQ[m][nx], db->stW[m][nx], xWA, xFl};
	hipLaunchKernelGGL(k_walk, dim3((S + 255) / 256), dim3(256), 0, st, wa);
	hipLaunchKernelGGL(k_maxc, dim3(nq), dim3(256), 0, st, S, (const int*)xWA, (const uint8_t*)xFl, xMinC, xNApp);
	ScoreArgs sa{nq, S, loop, qOff, dQWords, dQVals, xMinS, db->dRowOff, db->dRowLen, db->words, db->vals, xWA, xMinC, xFl, xSc};
	hipLaunchKernelGGL(k_score, dim3((S + 255) / 256, nq), dim3(256), 0, st, sa);
	hipLaunchKernelGGL(k_carry, dim3((S + 255) / 256), dim3(256), 0, st, nq, S, (const uint8_t*)xFl, xSc, db->stS[m][cu], db->stS[m][nx]);
	FinalArgs fa{nq, S, loop, xMinS, xMinC, xNApp, xWA, xFl, xSc, xMinw, db->dAddSeq, db->dId, db->dCovis, db->dCovisN, xLSlot, xLKey, xLAcc, xLBest, xLOrd, xSeen, cap,
	             xCand, xCandN, dcap, xDN, xDId, xDW, xDS, xDA, xDB};
	hipLaunchKernelGGL(k_final, dim3(nq), dim3(1024), 0, st, fa);
	HIPCHK(hipGetLastError());
	std::vector<int> candN(nq), dN(nq);
	int errv = 0;
	HIPCHK(hipMemcpyAsync(candN.data(), xCandN, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(dN.data(), xDN, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(&errv, err, 4, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	if (errv & 1) return fail(MCS_ERR_INVALID, "query BowVector: word id out of range");
	if (errv & 2) return fail(MCS_ERR_INVALID, "query BowVector: word ids must be strictly ascending");
	// outputs (counts are the full counts, also when they exceed the capacity)
	const hipMemcpyKind toUser = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
	int needC = 0, needD = 0;
	for (int q = 0; q < nq; ++q) { needC = std::max(needC, candN[q]); needD = std::max(needD, dN[q]); }
	if (host) memcpy(cand_count, candN.data(), (size_t)nq * 4);
	else HIPCHK(hipMemcpy(cand_count, candN.data(), (size_t)nq * 4, hipMemcpyHostToDevice));
	if (cap > 0) HIPCHK(hipMemcpy(cand_ids, xCand, (size_t)nq * cap * 8, toUser));
	if (diag && diag->count) {
		if (host) memcpy(diag->count, dN.data(), (size_t)nq * 4);
		else HIPCHK(hipMemcpy(diag->count, dN.data(), (size_t)nq * 4, hipMemcpyHostToDevice));
		if (dcap > 0) {
			const size_t nd = (size_t)nq * dcap;
			HIPCHK(hipMemcpy(diag->kf_id, xDId, nd * 8, toUser));
			HIPCHK(hipMemcpy(diag->words, xDW, nd * 4, toUser));
			HIPCHK(hipMemcpy(diag->score, xDS, nd * 8, toUser));
			HIPCHK(hipMemcpy(diag->acc, xDA, nd * 8, toUser));
			HIPCHK(hipMemcpy(diag->best, xDB, nd * 8, toUser));
		}
	}
	if (needC > cap) return fail(MCS_ERR_CAPACITY, "keyframe database: a query has " + std::to_string(needC) + " candidates, cap is " + std::to_string(cap) +
	                                                   " (cand_count holds the counts needed; the database state is unchanged)");
	if (diag && needD > dcap)
		return fail(MCS_ERR_CAPACITY, "keyframe database: a query scored " + std::to_string(needD) + " keyframes, diagnostics cap is " + std::to_string(dcap) +
		                                  " (the database state is unchanged)");
	db->cur[m] = nx;   // commit the state the batch left
	return MCS_OK;
}

int mcs_kfdb_detect_relocalisation(mcs_kfdb* db, int nq, const int64_t* query_ids, const int32_t* offsets, const int32_t* word_ids, const double* values,
                                   mcs_mem_kind kind, int cap, int32_t* cand_count, int64_t* cand_ids, const mcs_kfdb_diag* diag) {
	return kfdb_detect(db, 0, nq, query_ids, offsets, word_ids, values, nullptr, nullptr, nullptr, kind, cap, cand_count, cand_ids, diag);
}

int mcs_kfdb_detect_loop(mcs_kfdb* db, int nq, const int64_t* query_ids, const int32_t* offsets, const int32_t* word_ids, const double* values,
                         const int32_t* connected_offsets, const int64_t* connected_ids, const double* min_scores, mcs_mem_kind kind, int cap,
                         int32_t* cand_count, int64_t* cand_ids, const mcs_kfdb_diag* diag) {
	return kfdb_detect(db, 1, nq, query_ids, offsets, word_ids, values, connected_offsets, connected_ids, min_scores, kind, cap, cand_count, cand_ids, diag);
}

int mcs_kfdb_score(mcs_kfdb* db, int nw, const int32_t* word_ids, const double* values, int nkf, const int64_t* kf_ids, mcs_mem_kind kind, double* scores) {
	if (!db || nw < 0 || nkf < 0 || (nw && (!word_ids || !values)) || (nkf && (!kf_ids || !scores))) return fail(MCS_ERR_INVALID, "null argument");
	if (nkf == 0) return MCS_OK;
	mcs_ctx* c = db->ctx;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	const bool host = kind == MCS_MEM_HOST;
	std::vector<int64_t> ids;
	HIPCHK(fetch(ids, kf_ids, nkf, kind));
	std::vector<int> slots(nkf);
	for (int i = 0; i < nkf; ++i) {
		auto it = db->slotOf.find(ids[i]);
		if (it == db->slotOf.end() || !db->active[it->second])
			return fail(MCS_ERR_INVALID, "mcs_kfdb_score: keyframe " + std::to_string((long long)ids[i]) + " is not in the database");
		slots[i] = it->second;
	}
	if (host) {
		const int off[2] = {0, nw};
		if (int r = guard_bow_words(off, 1, word_ids, db->nWords, "mcs_kfdb_score")) return r;
	}
	int rc = kfdb_sync(db);
	if (rc != MCS_OK) return rc;
	const int *dSlots = nullptr, *dW = nullptr; const double* dV = nullptr; double* dOut = nullptr;
	Staging stg(c, host);
	stg.upload(&dSlots, slots.data(), (size_t)nkf * 4); stg.in(&dW, word_ids, (size_t)nw * 4); stg.in(&dV, values, (size_t)nw * 8); stg.out(&dOut, scores, (size_t)nkf * 8);
	if (int r = stg.commit()) return r;
	hipLaunchKernelGGL(k_score_list, dim3((nkf + 255) / 256), dim3(256), 0, st, dW, dV, nw, dSlots, nkf, db->dRowOff, db->dRowLen, db->words, db->vals, dOut);
	HIPCHK(hipGetLastError());
	return stg.finish(MCS_OK);
}

int mcs_vocabulary_set_words(mcs_vocabulary* v, const int32_t* word_id_per_node, const double* weight_per_node) {
	if (!v || !word_id_per_node || !weight_per_node) return fail(MCS_ERR_INVALID, "null argument");
	return mcs_vocabulary_set_words_internal(v, word_id_per_node, weight_per_node);
}

int mcs_bow_vector(mcs_vocabulary* v, const int32_t* leaf_nodes, int n, mcs_mem_kind kind, int32_t* word_ids_out, double* values_out, int32_t* nwords_out) {
	if (!v || n < 0 || (n && (!leaf_nodes || !word_ids_out || !values_out)) || !nwords_out) return fail(MCS_ERR_INVALID, "null argument");
	mcs_ctx* c = nullptr;
	int nNodes = 0, nWords = 0;
	int *wordOf = nullptr, *hist = nullptr;
	double* weightOf = nullptr;
	int rc = mcs_vocabulary_words_internal(v, &c, &nNodes, &wordOf, &weightOf, &hist, &nWords);
	if (rc != MCS_OK) return rc;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	const bool host = kind == MCS_MEM_HOST;
	const size_t nn = std::max(n, 1);
	// host kind: the outputs hold nwords_out entries, known only after the kernel, so they are fetched below from the block (intact until the next call)
	const int* dLeaf = nullptr; int *dW = nullptr, *outW = nullptr, *nOut = nullptr, *dErr = nullptr; double *dWt = nullptr, *outV = nullptr;
	int errv = 0, d = 0;
	Staging stg(c, host);
	stg.in(&dLeaf, leaf_nodes, (size_t)n * 4); stg.scratch(&dW, nn * 4); stg.scratch(&dWt, nn * 8); stg.download(&dErr, &errv, 4);
	if (host) { stg.scratch(&outW, nn * 4); stg.scratch(&outV, nn * 8); stg.download(&nOut, &d, 4); }
	else { outW = word_ids_out; outV = values_out; nOut = nwords_out; }
	if (int r = stg.commit()) return r;
	HIPCHK(hipMemsetAsync(dErr, 0, 4, st));
	hipLaunchKernelGGL(k_bow_vector, dim3(1), dim3(1024), 0, st, dLeaf, n, nNodes, nWords, wordOf, weightOf, hist, dW, dWt, outW, outV, nOut, dErr);
	HIPCHK(hipGetLastError());
	if (int r = stg.finish(MCS_OK)) return r;
	if (errv & 1) return fail(MCS_ERR_INVALID, "mcs_bow_vector: leaf node id out of range");
	if (errv & 2) return fail(MCS_ERR_INVALID, "mcs_bow_vector: a node with a weight > 0 has no word id (not a leaf)");
	if (host) {
		*nwords_out = d;
		if (d) {
			HIPCHK(hipMemcpy(word_ids_out, outW, (size_t)d * 4, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(values_out, outV, (size_t)d * 8, hipMemcpyDeviceToHost));
		}
	}
	return MCS_OK;
}
