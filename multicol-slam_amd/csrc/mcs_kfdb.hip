// mcs_kfdb.hip — cMultiKeyFrameDatabase (src/cMultiKeyFrameDatabase.cpp) on the device.  (The BowVector of a multi-frame, mcs_bow_vector, is in
// mcs_bow.hip with the vocabulary it reads.)
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
//
// Memory: the slab, the state arrays and the metadata are DevBufs of the database; the arrays of one call are a Staging on the context's block.  Slab and
// state grow with DevBuf::grow_keep to exactly the size of their schedule (slab max(need, 2 * capacity, 64) elements, state max(2 * slots, 256) slots): the
// hostile scripts count on WHICH call reallocates.  Every copy and fill is on the context's stream, like the kernels, and every call ends behind a
// synchronisation of it.
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

}  // namespace mcs

using namespace mcs;

namespace {

// copy n elements of a caller array (host or device) into a host vector; the device branch goes on the context's stream and waits for it
template <class T>
hipError_t fetch(std::vector<T>& dst, const T* src, size_t n, mcs_mem_kind kind, hipStream_t st) {
	dst.resize(n);
	if (!n) return hipSuccess;
	if (kind == MCS_MEM_HOST) { memcpy(dst.data(), src, n * sizeof(T)); return hipSuccess; }
	const hipError_t e = hipMemcpyAsync(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, st);
	return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// one output array of a detection call: `bytes` to the caller's array (host or device memory, by `host`) from a host vector (`fromHost`) or from a slot of the
// call's scratch.  Issued on the context's stream: the caller synchronises once, behind the last one.
hipError_t put(void* dst, const void* src, bool fromHost, size_t bytes, bool host, hipStream_t st) {
	if (!bytes) return hipSuccess;
	if (host && fromHost) { memcpy(dst, src, bytes); return hipSuccess; }
	return hipMemcpyAsync(dst, src, bytes, host ? hipMemcpyDeviceToHost : fromHost ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st);
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
	// the slab of rows: slabCap elements each, capacity max(need, 2 * slabCap, 64) when a row does not fit
	size_t slabUsed = 0, slabCap = 0;
	DevBuf words, vals;   // int / double
	// device copy of the slot metadata: one buffer, laid out and uploaded whole by kfdb_sync
	DevBuf meta;
	const int *dRowOff = nullptr, *dRowLen = nullptr, *dActive = nullptr, *dCovisN = nullptr, *dCovis = nullptr;
	const uint32_t* dAddSeq = nullptr; const int64_t* dId = nullptr;
	// persistent state, two copies each (current / next): [0] relocalisation, [1] loop; stCap slots each, capacity max(2 * slots, 256) when a slot does not fit
	struct State { DevBuf q, w, s; };   // int64_t query id, int word counter, double score
	int cur[2] = {0, 0};
	State st[2][2];
	size_t stCap = 0;
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

// room for `need` slab elements; the rows in use are kept
static hipError_t kfdb_slab(mcs_kfdb* db, size_t need) {
	if (need <= db->slabCap) return hipSuccess;
	const size_t nc = std::max<size_t>(std::max(need, db->slabCap * 2), 64);
	hipError_t e = db->words.grow_keep(nc * 4, db->slabUsed * 4, db->ctx->stream);
	if (e == hipSuccess) e = db->vals.grow_keep(nc * 8, db->slabUsed * 8, db->ctx->stream);
	if (e == hipSuccess) db->slabCap = nc;
	return e;
}

// device metadata and state arrays sized for every slot; new slots get the state of a keyframe never queried (query ids 0, counters 0, scores 0.0): the zero
// fill of grow_keep.  A growth that fails half way leaves stCap as it was, and the next call grows the arrays that are still short.
static int kfdb_sync(mcs_kfdb* db) {
	const size_t S = db->id.size();
	mcs_ctx* c = db->ctx;
	if (S > db->stCap) {
		const size_t nc = std::max<size_t>(S * 2, 256), old = db->stCap;
		for (int m = 0; m < 2; ++m)
			for (int b = 0; b < 2; ++b) {
				mcs_kfdb::State& x = db->st[m][b];
				HIPCHK(x.q.grow_keep(nc * 8, old * 8, c->stream)); HIPCHK(x.w.grow_keep(nc * 4, old * 4, c->stream)); HIPCHK(x.s.grow_keep(nc * 8, old * 8, c->stream));
			}
		db->stCap = nc;
	}
	if (!db->metaDirty) return MCS_OK;
	Staging stg(c, true);
	stg.upload(&db->dRowOff, db->rowOff.data(), S * 4); stg.upload(&db->dRowLen, db->rowLen.data(), S * 4); stg.upload(&db->dActive, db->active.data(), S * 4);
	stg.upload(&db->dCovisN, db->covisN.data(), S * 4); stg.upload(&db->dCovis, db->covis.data(), S * KF_COVIS * 4); stg.upload(&db->dAddSeq, db->addSeq.data(), S * 4);
	stg.upload(&db->dId, db->id.data(), S * 8);
	HIPCHK(db->meta.reserve(stg.bytes()));
	if (int r = stg.commit(db->meta.p)) return r;
	if (int r = stg.finish(MCS_OK)) return r;
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
		if (kfdb_slab(db, (size_t)capacity_hint * 1024) != hipSuccess) { delete db; return fail(MCS_ERR_HIP, "keyframe database allocation failed"); }
	}
	*out = db;
	return MCS_OK;
}

int mcs_kfdb_destroy(mcs_kfdb* db) {
	if (!db) return MCS_OK;
	(void)hipSetDevice(db->ctx->device);
	(void)hipStreamSynchronize(db->ctx->stream);
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
	hipStream_t st = db->ctx->stream;
	std::vector<int64_t> ids;
	std::vector<int> off, w;
	HIPCHK(fetch(ids, kf_ids, nkf, kind, st));
	HIPCHK(fetch(off, offsets, (size_t)nkf + 1, kind, st));
	if (int r = guard_bow_offsets(off.data(), nkf, "mcs_kfdb_add")) return r;   // before anything is sized by them
	const size_t total = (size_t)off[nkf];
	if (total && (!word_ids || !values)) return fail(MCS_ERR_INVALID, "null word / value array");
	HIPCHK(fetch(w, word_ids, total, kind, st));
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
	HIPCHK(kfdb_slab(db, base + total));
	if (total) {
		HIPCHK(hipMemcpyAsync(db->words.as<int>() + base, w.data(), total * 4, hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(db->vals.as<double>() + base, values, total * 8, kind == MCS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
		HIPCHK(hipStreamSynchronize(st));   // w and the caller's values are free again
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
	HIPCHK(fetch(off, offsets, (size_t)nq + 1, kind, st));
	if (int r = guard_bow_offsets(off.data(), nq, nullptr)) return r;
	const size_t total = (size_t)off[nq];
	if (total && (!word_ids || !values)) return fail(MCS_ERR_INVALID, "null word / value array");
	if (host)
		if (int r = guard_bow_words(off.data(), nq, word_ids, db->nWords, loop ? "mcs_kfdb_detect_loop" : "mcs_kfdb_detect_relocalisation")) return r;
	int rc = kfdb_sync(db);
	if (rc != MCS_OK) return rc;
	const int S = (int)db->id.size();
	std::vector<uint8_t> conn;
	if (loop && conn_offsets) {
		std::vector<int> coff;
		std::vector<int64_t> cids;
		HIPCHK(fetch(coff, conn_offsets, (size_t)nq + 1, kind, st));
		if (coff[0] != 0) return fail(MCS_ERR_INVALID, "connected offsets[0] must be 0");
		for (int q = 0; q < nq; ++q)
			if (coff[q + 1] < coff[q]) return fail(MCS_ERR_INVALID, "connected offsets must be non-decreasing");
		if (coff[nq] && !conn_ids) return fail(MCS_ERR_INVALID, "null connected ids");
		HIPCHK(fetch(cids, conn_ids, (size_t)coff[nq], kind, st));
		conn.assign((size_t)nq * std::max(S, 1), 0);
		for (int q = 0; q < nq; ++q)
			for (int k = coff[q]; k < coff[q + 1]; ++k) {
				auto it = db->slotOf.find(cids[k]);
				if (it != db->slotOf.end()) conn[(size_t)q * S + it->second] = 1;
			}
	}
	const size_t nq4 = (size_t)nq * 4;
	if (S == 0) {   // empty database: nothing shares a word
		const std::vector<int> z(nq, 0);
		HIPCHK(put(cand_count, z.data(), true, nq4, host, st));
		if (diag && diag->count) HIPCHK(put(diag->count, z.data(), true, nq4, host, st));
		HIPCHK(hipStreamSynchronize(st));
		return MCS_OK;
	}
	const int dcap = diag ? std::max(diag->cap, 0) : 0;
	const size_t NS = (size_t)nq * S, QC = (size_t)nq * std::max(cap, 1), QD = (size_t)nq * std::max(dcap, 1);
	// the call's arrays and scratch in the context's block: the connected matrix, made on the host, is uploaded; the caller's arrays are staged (host kind) or
	// read where they are (device kind: nothing goes to the host and back but the offsets, which size the call); the rest is scratch.  Candidates and
	// diagnostics land in scratch too: they reach the caller only when the query words are found good.
	uint32_t* bm = nullptr; int* xRes = nullptr; const int* qOff = nullptr; const int64_t* xQId = nullptr; const double* xMinS = nullptr; int* xMinC = nullptr;
	int* xNApp = nullptr; int* xCnt = nullptr; int* xMinw = nullptr; int* xWA = nullptr; uint8_t* xFl = nullptr; double* xSc = nullptr; uint8_t* xConn = nullptr;
	int* xLSlot = nullptr; uint64_t* xLKey = nullptr; double* xLAcc = nullptr; int* xLBest = nullptr; int* xLOrd = nullptr; uint8_t* xSeen = nullptr;
	int64_t* xCand = nullptr; int64_t* xDId = nullptr; int* xDW = nullptr; double* xDS = nullptr; double* xDA = nullptr;
	int64_t* xDB = nullptr; const int* dQWords = nullptr; const double* dQVals = nullptr;
	std::vector<int> res(2 * (size_t)nq + 1);   // what the host needs back, as one piece and one copy: candidate counts, diagnostic counts, the error word
	const int *candN = res.data(), *dN = candN + nq, &errv = res[2 * (size_t)nq];
	Staging stg(c, host);
	stg.upload(&xConn, conn.data(), loop ? NS : 1); stg.in(&qOff, offsets, ((size_t)nq + 1) * 4); stg.in(&xQId, query_ids, (size_t)nq * 8);
	stg.in(&xMinS, min_scores, (size_t)nq * 8); stg.in(&dQWords, word_ids, total * 4); stg.in(&dQVals, values, total * 8);
	stg.scratch(&bm, (size_t)nq * db->bmWords * 4); stg.scratch(&xMinC, nq4); stg.scratch(&xNApp, nq4); stg.scratch(&xCnt, NS * 4); stg.scratch(&xMinw, NS * 4);
	stg.scratch(&xWA, NS * 4); stg.scratch(&xFl, NS); stg.scratch(&xSc, NS * 8); stg.scratch(&xLSlot, NS * 4); stg.scratch(&xLKey, NS * 8); stg.scratch(&xLAcc, NS * 8);
	stg.scratch(&xLBest, NS * 4); stg.scratch(&xLOrd, NS * 4); stg.scratch(&xSeen, NS); stg.scratch(&xCand, QC * 8); stg.scratch(&xDId, QD * 8);
	stg.scratch(&xDW, QD * 4); stg.scratch(&xDS, QD * 8); stg.scratch(&xDA, QD * 8); stg.scratch(&xDB, QD * 8);
	stg.download(&xRes, res.data(), res.size() * 4);
	if (int r = stg.commit()) return r;
	int *xCandN = xRes, *xDN = xRes + nq, *err = xRes + 2 * (size_t)nq;
	if (loop && conn.empty()) HIPCHK(hipMemsetAsync(xConn, 0, NS, st));
	HIPCHK(hipMemsetAsync(bm, 0, (size_t)nq * db->bmWords * 4, st));
	HIPCHK(hipMemsetAsync(err, 0, 4, st));
	HIPCHK(hipMemsetAsync(xSeen, 0, NS, st));
	hipLaunchKernelGGL(k_qbitmap, dim3(nq), dim3(256), 0, st, qOff, dQWords, nq, db->nWords, db->bmWords, bm, err);
	const int* slabW = db->words.as<int>();
	CountArgs ca{bm, db->bmWords, nq, S, db->dRowOff, db->dRowLen, db->dActive, slabW, xCnt, xMinw};
	const size_t ldsBytes = (size_t)KF_QG * db->bmWords * 4;
	const dim3 gc((S + 3) / 4, (nq + KF_QG - 1) / KF_QG);
	if (ldsBytes <= (size_t)KF_LDS_BYTES) hipLaunchKernelGGL(k_count<true>, gc, dim3(256), ldsBytes, st, ca);
	else hipLaunchKernelGGL(k_count<false>, gc, dim3(256), 0, st, ca);
	const int m = loop ? 1 : 0;
	const int cu = db->cur[m], nx = 1 - cu;
	const mcs_kfdb::State &sc = db->st[m][cu], &sn = db->st[m][nx];
	WalkArgs wa{nq, S, loop, xQId, xConn, xCnt, sc.q.as<int64_t>(), sc.w.as<int>(), sn.q.as<int64_t>(), sn.w.as<int>(), xWA, xFl};
	hipLaunchKernelGGL(k_walk, dim3((S + 255) / 256), dim3(256), 0, st, wa);
	hipLaunchKernelGGL(k_maxc, dim3(nq), dim3(256), 0, st, S, (const int*)xWA, (const uint8_t*)xFl, xMinC, xNApp);
	ScoreArgs sa{nq, S, loop, qOff, dQWords, dQVals, xMinS, db->dRowOff, db->dRowLen, slabW, db->vals.as<double>(), xWA, xMinC, xFl, xSc};
	hipLaunchKernelGGL(k_score, dim3((S + 255) / 256, nq), dim3(256), 0, st, sa);
	hipLaunchKernelGGL(k_carry, dim3((S + 255) / 256), dim3(256), 0, st, nq, S, (const uint8_t*)xFl, xSc, (const double*)sc.s.as<double>(), sn.s.as<double>());
	FinalArgs fa{nq, S, loop, xMinS, xMinC, xNApp, xWA, xFl, xSc, xMinw, db->dAddSeq, db->dId, db->dCovis, db->dCovisN, xLSlot, xLKey, xLAcc, xLBest, xLOrd, xSeen, cap,
	             xCand, xCandN, dcap, xDN, xDId, xDW, xDS, xDA, xDB};
	hipLaunchKernelGGL(k_final, dim3(nq), dim3(1024), 0, st, fa);
	HIPCHK(hipGetLastError());
	if (int r = stg.finish(MCS_OK)) return r;   // candN, dN, errv are back; the block stays as it is until the next call
	if (errv & 1) return fail(MCS_ERR_INVALID, "query BowVector: word id out of range");
	if (errv & 2) return fail(MCS_ERR_INVALID, "query BowVector: word ids must be strictly ascending");
	// outputs (counts are the full counts, also when they exceed the capacity)
	int needC = 0, needD = 0;
	for (int q = 0; q < nq; ++q) { needC = std::max(needC, candN[q]); needD = std::max(needD, dN[q]); }
	HIPCHK(put(cand_count, host ? (const void*)candN : xCandN, host, nq4, host, st));
	HIPCHK(put(cand_ids, xCand, false, (size_t)nq * cap * 8, host, st));
	if (diag && diag->count) {
		const size_t nd = (size_t)nq * dcap;
		HIPCHK(put(diag->count, host ? (const void*)dN : xDN, host, nq4, host, st));
		HIPCHK(put(diag->kf_id, xDId, false, nd * 8, host, st)); HIPCHK(put(diag->words, xDW, false, nd * 4, host, st));
		HIPCHK(put(diag->score, xDS, false, nd * 8, host, st)); HIPCHK(put(diag->acc, xDA, false, nd * 8, host, st));
		HIPCHK(put(diag->best, xDB, false, nd * 8, host, st));
	}
	HIPCHK(hipStreamSynchronize(st));
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
	HIPCHK(fetch(ids, kf_ids, nkf, kind, st));
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
	hipLaunchKernelGGL(k_score_list, dim3((nkf + 255) / 256), dim3(256), 0, st, dW, dV, nw, dSlots, nkf, db->dRowOff, db->dRowLen, db->words.as<int>(),
	                   db->vals.as<double>(), dOut);
	HIPCHK(hipGetLastError());
	return stg.finish(MCS_OK);
}

