// mcs_covis.hip — the local map and the covisibility counts on the device:
//   cTracking::UpdateReferenceKeyFrames / UpdateReferencePoints   src/cTracking.cpp:1024-1123   (mcs_covis_update_reference)
//   cMultiKeyFrame::UpdateConnections (counting and ordering)      src/cMultiKeyFrame.cpp:406-500 (mcs_covis_update_connections)
// Both are "every map point of a voter row votes for the keyframes that observe it".  The store keeps one row of map point ids per keyframe (mvpMapPoints, -1 for
// NULL) and a DISTINCT copy of it (a repeated point replaced by -1: the reference's observations map holds a keyframe once per point).  A vote is then
//   mult[p]  = entries of the voter row equal to p whose point is not bad      (k_covis_mark: integer atomicAdd)
//   count[k] = sum of mult[p] over keyframe k's distinct row                   (k_covis_count: one wave per keyframe, plain loads, one store)
// Integer sums: any order gives the same result.  Where the reference orders by heap address (std::map<cMultiKeyFrame*, ...>) the store orders by mnId, which
// is slot order: a new keyframe's id exceeds every id present (DESIGN.md sections 4h and 7).
#include "mcs_host.h"
#include <unordered_map>

namespace mcs {
namespace {

constexpr unsigned long long kNoKey = ~0ull;

__device__ __forceinline__ int wave_sum(int v) {
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	return v;
}
__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// ---- rows
// row[i] = src[i] for i < n where it names a point, -1 otherwise and on the padding up to the pitch
__global__ __launch_bounds__(256) void k_covis_set_row(const int* src, int n, int maxPoints, int pitch, int* row) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= pitch) return;
	int v = i < n ? src[i] : -1;
	if ((unsigned)v >= (unsigned)maxPoints) v = -1;
	row[i] = v;
}
__global__ __launch_bounds__(256) void k_covis_first_index(const int* row, int n, unsigned long long* key) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = row[i];
	if (p >= 0) atomicMin(&key[p], (unsigned long long)i);
}
__global__ __launch_bounds__(256) void k_covis_distinct(const int* row, int n, int pitch, const unsigned long long* key, int* drow) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= pitch) return;
	const int p = i < n ? row[i] : -1;
	drow[i] = (p >= 0 && key[p] == (unsigned long long)i) ? p : -1;
}
__global__ __launch_bounds__(256) void k_covis_reset_row_keys(const int* row, int n, unsigned long long* key) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = row[i];
	if (p >= 0) key[p] = kNoKey;
}
__global__ void k_covis_meta(int slot, int n, int live, int bad, long long id, int what, int* rowN, uint8_t* liveF, uint8_t* badF, long long* ids, double* t) {
	if (threadIdx.x || blockIdx.x) return;
	if (what & 1) { rowN[slot] = n; liveF[slot] = (uint8_t)live; }
	if (what & 2) badF[slot] = (uint8_t)bad;
	if (what & 4) { ids[slot] = id; t[3 * slot] = 0.0; t[3 * slot + 1] = 0.0; t[3 * slot + 2] = 0.0; }
}
struct PoseSlots { int slot[32]; int n; };
__global__ void k_covis_pose(PoseSlots ps, const double* src, double* t) {
	const int i = threadIdx.x;
	if (i >= ps.n * 3) return;
	t[3 * ps.slot[i / 3] + i % 3] = src[i];
}
__global__ __launch_bounds__(256) void k_covis_points_bad(const int* ids, int n, const uint8_t* bad, int maxPoints, uint8_t* ptBad) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = ids[i];
	if ((unsigned)p < (unsigned)maxPoints) ptBad[p] = bad[i] ? 1 : 0;
}

// ---- the shared count
// One thread per voter feature: a point that is not bad votes once PER FEATURE (src/cTracking.cpp:1056-1071, src/cMultiKeyFrame.cpp:419-441).  nullBad: the
// frame's row is in/out, a bad point's entry becomes NULL (src/cTracking.cpp:1072-1075).
__global__ __launch_bounds__(256) void k_covis_mark(int* voter, int n, int maxPoints, const uint8_t* ptBad, int* mult, int nullBad) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = voter[i];
	if ((unsigned)p >= (unsigned)maxPoints) return;
	if (ptBad[p]) { if (nullBad) voter[i] = -1; }
	else atomicAdd(&mult[p], 1);
}
__global__ __launch_bounds__(256) void k_covis_unmark(const int* voter, int n, int maxPoints, int* mult) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = voter[i];
	if ((unsigned)p < (unsigned)maxPoints) mult[p] = 0;
}
// The hot kernel: one wave per keyframe slot streams the slot's distinct row once, 16 bytes per lane and load (rows are padded with -1 to a pitch of 4 entries
// and start 16-byte aligned), gathers mult[p] for every entry that names a point, and stores the wave's sum.  No atomics, no LDS.  `self`: the voter's own
// slot reads 0 (src/cMultiKeyFrame.cpp:435), as does an erased one.
__global__ __launch_bounds__(256) void k_covis_count(const int* __restrict__ drows, int pitch, const int* __restrict__ rowN, const uint8_t* __restrict__ live,
                                                      const int* __restrict__ mult, int nslots, int self, int* __restrict__ count) {
	const int slot = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (slot >= nslots) return;
	int sum = 0;
	if (live[slot] && slot != self) {
		const int n4 = (rowN[slot] + 3) >> 2;
		const int4* r = reinterpret_cast<const int4*>(drows + (size_t)slot * pitch);
		for (int j = lane; j < n4; j += 64) {
			const int4 v = r[j];
			if (v.x >= 0) sum += mult[v.x];
			if (v.y >= 0) sum += mult[v.y];
			if (v.z >= 0) sum += mult[v.z];
			if (v.w >= 0) sum += mult[v.w];
		}
	}
	sum = wave_sum(sum);
	if (lane == 0) count[slot] = sum;
}

// ---- UpdateReferenceKeyFrames, from :1079: one workgroup walks the slots in id order, 1024 at a time
__global__ __launch_bounds__(1024) void k_covis_local(const int* count, const uint8_t* live, const uint8_t* kfBad, const long long* ids, const double* kt,
                                                       const double* ft, int nslots, long long* localKfs, int* localW, double* localDist, int* nLocal,
                                                       long long* refKf, int* rankOf) {
	__shared__ int wtot[16];
	__shared__ int base;
	__shared__ unsigned long long best;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	if (tid == 0) { base = 0; best = 0; }
	__syncthreads();
	for (int s0 = 0; s0 < nslots; s0 += 1024) {
		const int k = s0 + tid;
		const bool in = k < nslots;
		const int cnt = in ? count[k] : 0;
		const bool loc = in && live[k] && cnt > 4 && !kfBad[k];   // :1098-1101
		const unsigned long long b = __ballot(loc);
		if (lane == 0) wtot[w] = __popcll(b);
		__syncthreads();
		int rank = base + __popcll(b & lanes_below());
		for (int j = 0; j < w; ++j) rank += wtot[j];
		if (in) rankOf[k] = loc ? rank : -1;
		if (loc) {
			const double dx = ft[0] - kt[3 * k], dy = ft[1] - kt[3 * k + 1], dz = ft[2] - kt[3 * k + 2];
			double s = 0;
			s += dx * dx; s += dy * dy; s += dz * dz;
			localKfs[rank] = ids[k]; localW[rank] = cnt; localDist[rank] = sqrt(s);   // :1108-1115
			atomicMax(&best, ((unsigned long long)cnt << 32) | (0xFFFFFFFFu - (unsigned)k));   // :1103-1107: the first, in id order, of the greatest count
		}
		__syncthreads();
		if (tid == 0) { int t = 0; for (int j = 0; j < 16; ++j) t += wtot[j]; base += t; }
		__syncthreads();
	}
	const int n = base;
	for (int k = n + tid; k < nslots; k += 1024) { localKfs[k] = -1; localW[k] = 0; localDist[k] = 0.0; }
	if (tid == 0) { *nLocal = n; *refKf = best ? ids[0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu)] : -1; }
}

// ---- UpdateReferencePoints: a point enters the list where the walk (local keyframes in order, features in order) meets it first, i.e. at its smallest key
// (local rank << 32) | feature.  One thread per (slot, feature); reset: put the touched keys back.
__global__ __launch_bounds__(256) void k_covis_first(const int* rows, int pitch, const int* rowN, const int* rankOf, const uint8_t* ptBad, unsigned long long* key,
                                                       int reset) {
	const int slot = blockIdx.x, f = blockIdx.y * 256 + threadIdx.x;
	const int r = rankOf[slot];
	if (r < 0 || f >= rowN[slot]) return;
	const int p = rows[(size_t)slot * pitch + f];
	if (p < 0 || ptBad[p]) return;   // :1038-1042
	if (reset) key[p] = kNoKey;
	else atomicMin(&key[p], ((unsigned long long)r << 32) | (unsigned)f);
}
// One wave per slot.  phase 0: cnt[slot] = first occurrences in the slot's row; phase 1: write them, in feature order, from off[slot] on.
__global__ __launch_bounds__(256) void k_covis_emit(const int* rows, int pitch, const int* rowN, const int* rankOf, const uint8_t* ptBad, const unsigned long long* key,
                                                      int nslots, int* cnt, const int* off, int* localPoints, int cap, int phase) {
	const int slot = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (slot >= nslots) return;
	const int r = rankOf[slot];
	const int n = r < 0 ? 0 : rowN[slot];
	int run = phase ? off[slot] : 0;
	const int* row = rows + (size_t)slot * pitch;
	for (int f0 = 0; f0 < n; f0 += 64) {
		const int f = f0 + lane;
		int p = -1;
		bool first = false;
		if (f < n) {
			p = row[f];
			first = p >= 0 && !ptBad[p] && key[p] == (((unsigned long long)r << 32) | (unsigned)f);
		}
		const unsigned long long b = __ballot(first);
		if (phase && first) {
			const int pos = run + __popcll(b & lanes_below());
			if (pos < cap) localPoints[pos] = p;
		}
		run += __popcll(b);
	}
	if (!phase && lane == 0) cnt[slot] = run;
}
// exclusive scan over the slots in one workgroup; *total = the sum
__global__ __launch_bounds__(1024) void k_covis_scan(const int* cnt, int nslots, int* off, int* total) {
	__shared__ int wtot[16];
	__shared__ int base;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	if (tid == 0) base = 0;
	__syncthreads();
	for (int s0 = 0; s0 < nslots; s0 += 1024) {
		const int k = s0 + tid;
		const int v = k < nslots ? cnt[k] : 0;
		int inc = v;
		for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
		if (lane == 63) wtot[w] = inc;
		__syncthreads();
		int pre = base + inc - v;
		for (int j = 0; j < w; ++j) pre += wtot[j];
		if (k < nslots) off[k] = pre;
		__syncthreads();
		if (tid == 0) { int t = 0; for (int j = 0; j < 16; ++j) t += wtot[j]; base += t; }
		__syncthreads();
	}
	if (tid == 0) *total = base;
}

// ---- UpdateConnections from :443: one workgroup per query.  vPairs = every keyframe with count >= th, or the single first-in-id-order maximum; ordered as
// sort() + push_front leave it: descending weight, ties by descending id (= slot).  Rank by counting.
__global__ __launch_bounds__(1024) void k_covis_order(const int* count, const long long* ids, int nslots, int th, int* nCounted, long long* ordered, int* orderedW,
                                                       int* nOrdered) {
	__shared__ int nz, nth;
	__shared__ unsigned long long best;
	const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
	const int* c = count + (size_t)q * nslots;
	long long* ord = ordered + (size_t)q * nslots;
	int* ow = orderedW + (size_t)q * nslots;
	if (tid == 0) { nz = 0; nth = 0; best = 0; }
	__syncthreads();
	int z = 0, t = 0;
	unsigned long long b = 0;
	for (int k = tid; k < nslots; k += 1024) {
		const int v = c[k];
		if (v > 0) {
			++z;
			if (v >= th) ++t;
			const unsigned long long key = ((unsigned long long)v << 32) | (0xFFFFFFFFu - (unsigned)k);   // :457-461: strictly greater, so the first of the maximum
			if (key > b) b = key;
		}
	}
	z = wave_sum(z); t = wave_sum(t);
	for (int o = 32; o > 0; o >>= 1) { const unsigned long long x = __shfl_xor(b, o); if (x > b) b = x; }
	if (lane == 0) { if (z) atomicAdd(&nz, z); if (t) atomicAdd(&nth, t); if (b) atomicMax(&best, b); }
	__syncthreads();
	const int counted = nz, above = nth;
	int n = 0;
	if (counted > 0) {
		if (above > 0) {
			n = above;
			for (int k = tid; k < nslots; k += 1024) {
				const int v = c[k];
				if (v < th) continue;
				int rank = 0;
				for (int j = 0; j < nslots; ++j) {
					const int u = c[j];
					rank += (u > v || (u == v && j > k)) ? 1 : 0;   // u > v >= th, or u == v >= th: j is in vPairs too
				}
				ord[rank] = ids[k]; ow[rank] = v;
			}
		} else {
			n = 1;
			if (tid == 0) { ord[0] = ids[0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu)]; ow[0] = (int)(best >> 32); }   // :469-473
		}
	}
	for (int k = n + tid; k < nslots; k += 1024) { ord[k] = -1; ow[k] = 0; }
	if (tid == 0) { nCounted[q] = counted; nOrdered[q] = counted > 0 ? n : -1; }   // :443-444: an empty KFcounter leaves the old lists
}

// ---- row gather / scatter (units of W bytes)
struct FillRow { uint32_t w[64]; };
template <class W>
__global__ __launch_bounds__(256) void k_gather_rows(const int* idx, long long total, int upr, const W* src, FillRow fill, W* dst) {
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
	if (t >= total) return;
	const long long i = t / upr;
	const int j = (int)(t - i * upr);
	const int k = idx[i];
	dst[t] = k >= 0 ? src[(long long)k * upr + j] : reinterpret_cast<const W*>(fill.w)[j];
}
template <class W>
__global__ __launch_bounds__(256) void k_scatter_rows(const int* idx, long long total, int upr, const W* src, W* dst) {
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
	if (t >= total) return;
	const long long i = t / upr;
	const int j = (int)(t - i * upr);
	const int k = idx[i];
	if (k >= 0) dst[(long long)k * upr + j] = src[t];
}

inline unsigned blocks(long long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

}  // namespace
}  // namespace mcs

using namespace mcs;

struct mcs_covis {
	mcs_ctx* ctx = nullptr;
	int maxKf = 0, maxFeat = 0, maxPts = 0, pitch = 0;
	// host view of the slots: ids ascending, erased ones stay as holes until mcs_covis_clear
	std::vector<int64_t> id;
	std::vector<uint8_t> live;
	std::vector<int> rowN;
	std::unordered_map<int64_t, int> slotOf;
	int nLive = 0;
	// device
	DevBuf mem;
	int* rows = nullptr; int* drows = nullptr; int* dRowN = nullptr; uint8_t* dLive = nullptr; uint8_t* dKfBad = nullptr; long long* dIds = nullptr; double* dT = nullptr;
	uint8_t* ptBad = nullptr; int* mult = nullptr; unsigned long long* key = nullptr;
	int* count = nullptr; int* cnt = nullptr; int* off = nullptr; int* rankOf = nullptr;
};

static int covis_slot(const mcs_covis* h, int64_t id) {
	auto it = h->slotOf.find(id);
	return (it == h->slotOf.end() || !h->live[it->second]) ? -1 : it->second;
}

int mcs_covis_create(mcs_ctx* c, int max_keyframes, int max_features, int max_points, mcs_covis** out) {
	if (!c || !out) return fail(MCS_ERR_INVALID, "null argument");
	if (max_keyframes < 1 || max_features < 1 || max_points < 1 || max_keyframes > (1 << 24) || max_features > (1 << 20))
		return fail(MCS_ERR_INVALID, "capacities must be >= 1 (keyframes <= 2^24, features <= 2^20)");
	HIPCHK(hipSetDevice(c->device));
	mcs_covis* h = new mcs_covis();
	h->ctx = c; h->maxKf = max_keyframes; h->maxFeat = max_features; h->maxPts = max_points;
	h->pitch = (max_features + 3) / 4 * 4;   // rows start 16-byte aligned
	const size_t K = (size_t)max_keyframes, P = (size_t)max_points, rowBytes = K * h->pitch * 4;
	Carve cv;
	const size_t oRows = cv.take(rowBytes), oDrows = cv.take(rowBytes), oN = cv.take(K * 4), oLive = cv.take(K), oBad = cv.take(K), oIds = cv.take(K * 8),
	             oT = cv.take(K * 24), oPt = cv.take(P), oMult = cv.take(P * 4), oKey = cv.take(P * 8), oCount = cv.take(K * 4), oCnt = cv.take(K * 4),
	             oOff = cv.take(K * 4), oRank = cv.take(K * 4);
	const hipError_t e = h->mem.reserve(cv.total);
	if (e != hipSuccess) { delete h; return fail(MCS_ERR_HIP, std::string("covisibility store allocation failed: ") + hipGetErrorString(e)); }
	uint8_t* b = h->mem.p;
	h->rows = (int*)(b + oRows); h->drows = (int*)(b + oDrows); h->dRowN = (int*)(b + oN); h->dLive = b + oLive; h->dKfBad = b + oBad;
	h->dIds = (long long*)(b + oIds); h->dT = (double*)(b + oT); h->ptBad = b + oPt; h->mult = (int*)(b + oMult); h->key = (unsigned long long*)(b + oKey);
	h->count = (int*)(b + oCount); h->cnt = (int*)(b + oCnt); h->off = (int*)(b + oOff); h->rankOf = (int*)(b + oRank);
	hipError_t e2 = hipMemsetAsync(b, 0, cv.total, c->stream);
	if (e2 == hipSuccess) e2 = hipMemsetAsync(h->key, 0xFF, P * 8, c->stream);
	if (e2 == hipSuccess) e2 = hipStreamSynchronize(c->stream);
	if (e2 != hipSuccess) { delete h; return fail(MCS_ERR_HIP, std::string("covisibility store initialisation failed: ") + hipGetErrorString(e2)); }
	*out = h;
	return MCS_OK;
}

int mcs_covis_destroy(mcs_covis* h) {
	if (!h) return MCS_OK;
	(void)hipSetDevice(h->ctx->device);
	(void)hipStreamSynchronize(h->ctx->stream);
	delete h;
	return MCS_OK;
}

int mcs_covis_clear(mcs_covis* h) {
	if (!h) return fail(MCS_ERR_INVALID, "null argument");
	HIPCHK(hipSetDevice(h->ctx->device));
	HIPCHK(hipMemsetAsync(h->ptBad, 0, (size_t)h->maxPts, h->ctx->stream));   // the flags of the map points go with the keyframes
	h->id.clear(); h->live.clear(); h->rowN.clear(); h->slotOf.clear(); h->nLive = 0;
	return MCS_OK;
}

int mcs_covis_size(const mcs_covis* h, int* n) {
	if (!h || !n) return fail(MCS_ERR_INVALID, "null argument");
	*n = h->nLive;
	return MCS_OK;
}

int mcs_covis_slots(const mcs_covis* h, int* n) {
	if (!h || !n) return fail(MCS_ERR_INVALID, "null argument");
	*n = (int)h->id.size();
	return MCS_OK;
}

int mcs_covis_set_keyframe(mcs_covis* h, int64_t mnId, const int32_t* points, int n, mcs_mem_kind kind) {
	if (!h || (n > 0 && !points)) return fail(MCS_ERR_INVALID, "null argument");
	if (n < 0 || mnId < 0) return fail(MCS_ERR_INVALID, "bad keyframe id / feature count");
	if (n > h->maxFeat) return fail(MCS_ERR_CAPACITY, "more features than the store's max_features");
	auto it = h->slotOf.find(mnId);
	int slot = -1;
	if (it != h->slotOf.end()) {
		if (!h->live[it->second]) return fail(MCS_ERR_INVALID, "this keyframe id was erased: a new keyframe's id must exceed every id present");
		slot = it->second;
	} else {
		if (!h->id.empty() && mnId <= h->id.back()) return fail(MCS_ERR_INVALID, "a new keyframe's id must exceed every id present");
		if ((int)h->id.size() >= h->maxKf) return fail(MCS_ERR_CAPACITY, "more keyframes than the store's max_keyframes");
	}
	if (kind == MCS_MEM_HOST)
		for (int i = 0; i < n; ++i)
			if (points[i] < -1 || points[i] >= h->maxPts) return fail(MCS_ERR_INVALID, "map point id outside [-1, max_points)");
	mcs_ctx* c = h->ctx;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	Staging st(c, kind == MCS_MEM_HOST);
	const int* src = nullptr;
	st.in(&src, points, (size_t)n * 4);
	if (int r = st.commit()) return r;
	const bool isNew = slot < 0;
	if (isNew) {
		slot = (int)h->id.size();
		h->id.push_back(mnId); h->live.push_back(1); h->rowN.push_back(n); h->slotOf[mnId] = slot; ++h->nLive;
	} else h->rowN[slot] = n;
	int* row = h->rows + (size_t)slot * h->pitch;
	int* drow = h->drows + (size_t)slot * h->pitch;
	const unsigned gp = blocks(h->pitch);
	hipLaunchKernelGGL(k_covis_set_row, dim3(gp), dim3(256), 0, s, src, n, h->maxPts, h->pitch, row);
	if (n > 0) hipLaunchKernelGGL(k_covis_first_index, dim3(blocks(n)), dim3(256), 0, s, (const int*)row, n, h->key);
	hipLaunchKernelGGL(k_covis_distinct, dim3(gp), dim3(256), 0, s, (const int*)row, n, h->pitch, (const unsigned long long*)h->key, drow);
	if (n > 0) hipLaunchKernelGGL(k_covis_reset_row_keys, dim3(blocks(n)), dim3(256), 0, s, (const int*)row, n, h->key);
	hipLaunchKernelGGL(k_covis_meta, dim3(1), dim3(1), 0, s, slot, n, 1, 0, (long long)mnId, isNew ? 7 : 1, h->dRowN, h->dLive, h->dKfBad, h->dIds, h->dT);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_covis_set_keyframe_pose(mcs_covis* h, int n, const int64_t* mnIds, const double* t, mcs_mem_kind kind) {
	if (!h || n < 0 || (n > 0 && (!mnIds || !t))) return fail(MCS_ERR_INVALID, "null argument");
	std::vector<int> slots(n);
	for (int i = 0; i < n; ++i)
		if ((slots[i] = covis_slot(h, mnIds[i])) < 0) return fail(MCS_ERR_INVALID, "keyframe not in the store");
	if (n == 0) return MCS_OK;
	mcs_ctx* c = h->ctx;
	HIPCHK(hipSetDevice(c->device));
	Staging st(c, kind == MCS_MEM_HOST);
	const double* src = nullptr;
	st.in(&src, t, (size_t)n * 24);
	if (int r = st.commit()) return r;
	for (int i0 = 0; i0 < n; i0 += 32) {
		PoseSlots ps;
		ps.n = std::min(32, n - i0);
		for (int k = 0; k < 32; ++k) ps.slot[k] = k < ps.n ? slots[i0 + k] : 0;
		hipLaunchKernelGGL(k_covis_pose, dim3(1), dim3(128), 0, c->stream, ps, src + 3 * (size_t)i0, h->dT);
	}
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_covis_erase_keyframe(mcs_covis* h, int64_t mnId) {
	if (!h) return fail(MCS_ERR_INVALID, "null argument");
	const int slot = covis_slot(h, mnId);
	if (slot < 0) return fail(MCS_ERR_INVALID, "keyframe not in the store");
	HIPCHK(hipSetDevice(h->ctx->device));
	hipLaunchKernelGGL(k_covis_meta, dim3(1), dim3(1), 0, h->ctx->stream, slot, 0, 0, 0, 0ll, 1, h->dRowN, h->dLive, h->dKfBad, h->dIds, h->dT);
	HIPCHK(hipGetLastError());
	h->live[slot] = 0; h->rowN[slot] = 0; --h->nLive;
	return MCS_OK;
}

int mcs_covis_set_keyframe_bad(mcs_covis* h, int64_t mnId, int bad) {
	if (!h) return fail(MCS_ERR_INVALID, "null argument");
	const int slot = covis_slot(h, mnId);
	if (slot < 0) return fail(MCS_ERR_INVALID, "keyframe not in the store");
	HIPCHK(hipSetDevice(h->ctx->device));
	hipLaunchKernelGGL(k_covis_meta, dim3(1), dim3(1), 0, h->ctx->stream, slot, 0, 0, bad ? 1 : 0, 0ll, 2, h->dRowN, h->dLive, h->dKfBad, h->dIds, h->dT);
	HIPCHK(hipGetLastError());
	return MCS_OK;
}

int mcs_covis_set_points_bad(mcs_covis* h, const int32_t* ids, int n, const uint8_t* bad, mcs_mem_kind kind) {
	if (!h || n < 0 || (n > 0 && (!ids || !bad))) return fail(MCS_ERR_INVALID, "null argument");
	if (n == 0) return MCS_OK;
	if (kind == MCS_MEM_HOST)
		for (int i = 0; i < n; ++i)
			if (ids[i] < 0 || ids[i] >= h->maxPts) return fail(MCS_ERR_INVALID, "map point id outside [0, max_points)");
	mcs_ctx* c = h->ctx;
	HIPCHK(hipSetDevice(c->device));
	Staging st(c, kind == MCS_MEM_HOST);
	const int* dIds = nullptr; const uint8_t* dBad = nullptr;
	st.in(&dIds, ids, (size_t)n * 4); st.in(&dBad, bad, (size_t)n);
	if (int r = st.commit()) return r;
	hipLaunchKernelGGL(k_covis_points_bad, dim3(blocks(n)), dim3(256), 0, c->stream, dIds, n, dBad, h->maxPts, h->ptBad);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

// mark / count / unmark of one voter row on stream s; the scratch is clean again behind it
static void covis_vote(mcs_covis* h, int* voter, int n, int nullBad, int self, int S, int* count, hipStream_t s) {
	if (n > 0) hipLaunchKernelGGL(k_covis_mark, dim3(blocks(n)), dim3(256), 0, s, voter, n, h->maxPts, (const uint8_t*)h->ptBad, h->mult, nullBad);
	if (S > 0) {
		h->ctx->tic("covis_count");
		hipLaunchKernelGGL(k_covis_count, dim3(blocks((long long)S * 64)), dim3(256), 0, s, (const int*)h->drows, h->pitch, (const int*)h->dRowN,
		                   (const uint8_t*)h->dLive, (const int*)h->mult, S, self, count);
		h->ctx->toc("covis_count");
	}
	if (n > 0) hipLaunchKernelGGL(k_covis_unmark, dim3(blocks(n)), dim3(256), 0, s, (const int*)voter, n, h->maxPts, h->mult);
}

int mcs_covis_update_reference(mcs_covis* h, int32_t* frame_points, int nf, const double* frame_t, int cap, mcs_mem_kind kind, int64_t* local_kfs,
                               int32_t* local_weights, double* local_dist, int32_t* n_local, int64_t* ref_kf, int32_t* local_points, int32_t* n_points) {
	if (!h || !frame_t || !n_local || !ref_kf || !n_points || (nf > 0 && !frame_points) || (cap > 0 && !local_points)) return fail(MCS_ERR_INVALID, "null argument");
	if (nf < 0 || cap < 0) return fail(MCS_ERR_INVALID, "bad sizes");
	const int S = (int)h->id.size();
	if (S > 0 && (!local_kfs || !local_weights || !local_dist)) return fail(MCS_ERR_INVALID, "null argument");
	mcs_ctx* c = h->ctx;
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the local map is built in order: switch deferred searches off (mcs_ctx_set_async_search)");
	if (kind == MCS_MEM_HOST)
		for (int i = 0; i < nf; ++i)
			if (frame_points[i] < -1 || frame_points[i] >= h->maxPts) return fail(MCS_ERR_INVALID, "map point id outside [-1, max_points)");
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	if (int r = ctx_join_greedy(c, s)) return r;   // the frame's row may come from a search whose greedy pass runs on the side stream
	Staging st(c, kind == MCS_MEM_HOST);
	int* fp = nullptr; const double* ft = nullptr;
	long long* oKfs = nullptr; int* oW = nullptr; double* oD = nullptr; int* oNl = nullptr; long long* oRef = nullptr; int* oLp = nullptr; int* oNp = nullptr;
	st.inout(&fp, frame_points, (size_t)nf * 4); st.in(&ft, frame_t, 24);
	st.out(&oKfs, local_kfs, (size_t)S * 8); st.out(&oW, local_weights, (size_t)S * 4); st.out(&oD, local_dist, (size_t)S * 8);
	st.out(&oNl, n_local, 4); st.out(&oRef, ref_kf, 8); st.out(&oLp, local_points, (size_t)cap * 4); st.out(&oNp, n_points, 4);
	if (int r = st.commit()) return r;
	covis_vote(h, fp, nf, 1, -1, S, h->count, s);
	hipLaunchKernelGGL(k_covis_local, dim3(1), dim3(1024), 0, s, (const int*)h->count, (const uint8_t*)h->dLive, (const uint8_t*)h->dKfBad, (const long long*)h->dIds,
	                   (const double*)h->dT, ft, S, oKfs, oW, oD, oNl, oRef, h->rankOf);
	if (cap > 0) HIPCHK(hipMemsetAsync(oLp, 0xFF, (size_t)cap * 4, s));
	if (S > 0) {
		const dim3 gf((unsigned)S, blocks(h->pitch));
		const unsigned gw = blocks((long long)S * 64);
		hipLaunchKernelGGL(k_covis_first, gf, dim3(256), 0, s, (const int*)h->rows, h->pitch, (const int*)h->dRowN, (const int*)h->rankOf, (const uint8_t*)h->ptBad, h->key, 0);
		hipLaunchKernelGGL(k_covis_emit, dim3(gw), dim3(256), 0, s, (const int*)h->rows, h->pitch, (const int*)h->dRowN, (const int*)h->rankOf, (const uint8_t*)h->ptBad,
		                   (const unsigned long long*)h->key, S, h->cnt, (const int*)h->off, oLp, cap, 0);
	}
	hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(1024), 0, s, (const int*)h->cnt, S, h->off, oNp);
	if (S > 0) {
		const dim3 gf((unsigned)S, blocks(h->pitch));
		const unsigned gw = blocks((long long)S * 64);
		hipLaunchKernelGGL(k_covis_emit, dim3(gw), dim3(256), 0, s, (const int*)h->rows, h->pitch, (const int*)h->dRowN, (const int*)h->rankOf, (const uint8_t*)h->ptBad,
		                   (const unsigned long long*)h->key, S, h->cnt, (const int*)h->off, oLp, cap, 1);
		hipLaunchKernelGGL(k_covis_first, gf, dim3(256), 0, s, (const int*)h->rows, h->pitch, (const int*)h->dRowN, (const int*)h->rankOf, (const uint8_t*)h->ptBad, h->key, 1);
	}
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_covis_update_connections(mcs_covis* h, int nq, const int64_t* mnIds, mcs_mem_kind kind, int32_t* count, int32_t* n_counted, int64_t* ordered,
                                 int32_t* ordered_w, int32_t* n_ordered) {
	if (!h || nq < 0 || (nq > 0 && (!mnIds || !count || !n_counted || !ordered || !ordered_w || !n_ordered))) return fail(MCS_ERR_INVALID, "null argument");
	mcs_ctx* c = h->ctx;
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the covisibility counts run in order: switch deferred searches off (mcs_ctx_set_async_search)");
	const int S = (int)h->id.size();
	std::vector<int> slots(nq);
	for (int q = 0; q < nq; ++q)
		if ((slots[q] = covis_slot(h, mnIds[q])) < 0) return fail(MCS_ERR_INVALID, "keyframe not in the store");
	if (nq == 0) return MCS_OK;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	Staging st(c, kind == MCS_MEM_HOST);
	int* oC = nullptr; int* oN = nullptr; long long* oO = nullptr; int* oW = nullptr; int* oNo = nullptr;
	const size_t QS = (size_t)nq * S;
	st.out(&oC, count, QS * 4); st.out(&oN, n_counted, (size_t)nq * 4); st.out(&oO, ordered, QS * 8); st.out(&oW, ordered_w, QS * 4); st.out(&oNo, n_ordered, (size_t)nq * 4);
	if (int r = st.commit()) return r;
	for (int q = 0; q < nq; ++q)   // the rows do not change: a batch equals the sequence
		covis_vote(h, h->rows + (size_t)slots[q] * h->pitch, h->rowN[slots[q]], 0, slots[q], S, oC + (size_t)q * S, s);
	hipLaunchKernelGGL(k_covis_order, dim3(nq), dim3(1024), 0, s, (const int*)oC, (const long long*)h->dIds, S, 30, oN, oO, oW, oNo);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

// ---- device helpers
static int row_unit(const void* a, const void* b, int rowBytes) {
	const uintptr_t m = (uintptr_t)a | (uintptr_t)b | (uintptr_t)rowBytes;
	return (m & 15) == 0 ? 16 : (m & 7) == 0 ? 8 : (m & 3) == 0 ? 4 : 1;
}

int mcs_gather_rows(mcs_ctx* c, const int32_t* idx, int n, const void* src, int row_bytes, const void* fill_row, void* dst) {
	if (!c || n < 0 || row_bytes < 1 || (n > 0 && (!idx || !src || !dst))) return fail(MCS_ERR_INVALID, "null argument / bad sizes");
	if (row_bytes > (int)sizeof(FillRow)) return fail(MCS_ERR_UNSUPPORTED, "rows of more than 256 bytes");
	if (n == 0) return MCS_OK;
	HIPCHK(hipSetDevice(c->device));
	FillRow fill;
	memset(&fill, 0, sizeof(fill));
	if (fill_row) memcpy(&fill, fill_row, row_bytes);
	const int u = row_unit(src, dst, row_bytes), upr = row_bytes / u;
	const long long total = (long long)n * upr;
	const dim3 g(blocks(total)), b(256);
	if (u == 16) hipLaunchKernelGGL(k_gather_rows<uint4>, g, b, 0, c->stream, idx, total, upr, (const uint4*)src, fill, (uint4*)dst);
	else if (u == 8) hipLaunchKernelGGL(k_gather_rows<uint2>, g, b, 0, c->stream, idx, total, upr, (const uint2*)src, fill, (uint2*)dst);
	else if (u == 4) hipLaunchKernelGGL(k_gather_rows<uint32_t>, g, b, 0, c->stream, idx, total, upr, (const uint32_t*)src, fill, (uint32_t*)dst);
	else hipLaunchKernelGGL(k_gather_rows<uint8_t>, g, b, 0, c->stream, idx, total, upr, (const uint8_t*)src, fill, (uint8_t*)dst);
	HIPCHK(hipGetLastError());
	return MCS_OK;
}

int mcs_scatter_rows(mcs_ctx* c, const int32_t* idx, int n, const void* src, int row_bytes, void* dst) {
	if (!c || n < 0 || row_bytes < 1 || (n > 0 && (!idx || !src || !dst))) return fail(MCS_ERR_INVALID, "null argument / bad sizes");
	if (n == 0) return MCS_OK;
	HIPCHK(hipSetDevice(c->device));
	const int u = row_unit(src, dst, row_bytes), upr = row_bytes / u;
	const long long total = (long long)n * upr;
	const dim3 g(blocks(total)), b(256);
	if (u == 16) hipLaunchKernelGGL(k_scatter_rows<uint4>, g, b, 0, c->stream, idx, total, upr, (const uint4*)src, (uint4*)dst);
	else if (u == 8) hipLaunchKernelGGL(k_scatter_rows<uint2>, g, b, 0, c->stream, idx, total, upr, (const uint2*)src, (uint2*)dst);
	else if (u == 4) hipLaunchKernelGGL(k_scatter_rows<uint32_t>, g, b, 0, c->stream, idx, total, upr, (const uint32_t*)src, (uint32_t*)dst);
	else hipLaunchKernelGGL(k_scatter_rows<uint8_t>, g, b, 0, c->stream, idx, total, upr, (const uint8_t*)src, (uint8_t*)dst);
	HIPCHK(hipGetLastError());
	return MCS_OK;
}
