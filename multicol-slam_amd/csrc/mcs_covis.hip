// mcs_covis.hip — the local map and the covisibility counts on the device:
//   cTracking::UpdateReferenceKeyFrames / UpdateReferencePoints   src/cTracking.cpp:1024-1123   (mcs_covis_update_reference)
//   cMultiKeyFrame::UpdateConnections (counting and ordering)      src/cMultiKeyFrame.cpp:406-500 (mcs_covis_update_connections)
// and the store itself (mcs_covis.h); culling lives in mcs_cull.hip, refreshing map points in mcs_mappoints.hip.
// Both are "every map point of a voter row votes for the keyframes that observe it".  The store keeps one row of map point ids per keyframe (mvpMapPoints, -1 for
// NULL) and a DISTINCT copy of it (a repeated point replaced by -1: the reference's observations map holds a keyframe once per point).  A vote is then
//   mult[p]  = entries of the voter row equal to p whose point is not bad      (k_covis_mark: integer atomicAdd)
//   count[k] = sum of mult[p] over keyframe k's distinct row                   (k_covis_count: one wave per keyframe, plain loads, one store)
// Integer sums: any order gives the same result.  Where the reference orders by heap address (std::map<cMultiKeyFrame*, ...>) the store orders by mnId, which
// is slot order: a new keyframe's id exceeds every id present (DESIGN.md sections 4h and 7).
#include "mcs_covis.h"

namespace mcs {

__global__ __launch_bounds__(256) void k_covis_unmark(const int* voter, int n, int maxPoints, int* mult) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = voter[i];
	if ((unsigned)p < (unsigned)maxPoints) mult[p] = 0;
}
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
		const int pre = block_before(wtot, base) + inc - v;
		if (k < nslots) off[k] = pre;
		block_carry(wtot, base);
	}
	if (tid == 0) *total = base;
}

namespace {

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
// The hot kernel: one wave per keyframe slot streams the slot's distinct row once (walk_row), gathers mult[p] for every entry that names a point, and stores
// the wave's sum.  No atomics, no LDS.  `self`: the voter's own slot reads 0 (src/cMultiKeyFrame.cpp:435), as does an erased one.
__global__ __launch_bounds__(256) void k_covis_count(CovisView s, const int* __restrict__ mult, int self, int* __restrict__ count) {
	const int slot = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (slot >= s.nslots) return;
	int sum = 0;
	if (s.live[slot] && slot != self) walk_row<false>(s.drow(slot), nullptr, s.rowN[slot], lane, [&](int p, int, int, unsigned) { sum += mult[p]; });
	sum = wave_sum(sum);
	if (lane == 0) count[slot] = sum;
}

// ---- UpdateReferenceKeyFrames, from :1079: one workgroup walks the slots in id order, 1024 at a time
__global__ __launch_bounds__(1024) void k_covis_local(CovisView s, const int* count, const double* ft, long long* localKfs, int* localW, double* localDist, int* nLocal,
                                                       long long* refKf, int* rankOf) {
	__shared__ int wtot[16];
	__shared__ int base;
	__shared__ unsigned long long best;
	const int tid = threadIdx.x, nslots = s.nslots;
	if (tid == 0) { base = 0; best = 0; }
	__syncthreads();
	for (int s0 = 0; s0 < nslots; s0 += 1024) {
		const int k = s0 + tid;
		const bool in = k < nslots;
		const int cnt = in ? count[k] : 0;
		const bool loc = in && s.live[k] && cnt > 4 && !s.kfBad[k];   // :1098-1101
		const int rank = block_rank(loc, wtot, base);
		if (in) rankOf[k] = loc ? rank : -1;
		if (loc) {
			const double dx = ft[0] - s.t[3 * k], dy = ft[1] - s.t[3 * k + 1], dz = ft[2] - s.t[3 * k + 2];
			double d = 0;
			d += dx * dx; d += dy * dy; d += dz * dz;
			localKfs[rank] = s.ids[k]; localW[rank] = cnt; localDist[rank] = sqrt(d);   // :1108-1115
			atomicMax(&best, ((unsigned long long)cnt << 32) | (0xFFFFFFFFu - (unsigned)k));   // :1103-1107: the first, in id order, of the greatest count
		}
		block_carry(wtot, base);
	}
	const int n = base;
	for (int k = n + tid; k < nslots; k += 1024) { localKfs[k] = -1; localW[k] = 0; localDist[k] = 0.0; }
	if (tid == 0) { *nLocal = n; *refKf = best ? s.ids[0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu)] : -1; }
}

// ---- UpdateReferencePoints: a point enters the list where the walk (local keyframes in order, features in order) meets it first, i.e. at its smallest key
// (local rank << 32) | feature.  One thread per (slot, feature); reset: put the touched keys back.
__global__ __launch_bounds__(256) void k_covis_first(CovisView s, const int* rankOf, unsigned long long* key, int reset) {
	const int slot = blockIdx.x, f = blockIdx.y * 256 + threadIdx.x;
	const int r = rankOf[slot];
	if (r < 0 || f >= s.rowN[slot]) return;
	const int p = s.row(slot)[f];
	if (p < 0 || s.ptBad[p]) return;   // :1038-1042
	if (reset) key[p] = kNoKey;
	else atomicMin(&key[p], ((unsigned long long)r << 32) | (unsigned)f);
}
// One wave per slot.  phase 0: cnt[slot] = first occurrences in the slot's row; phase 1: write them, in feature order, from off[slot] on.
__global__ __launch_bounds__(256) void k_covis_emit(CovisView s, const int* rankOf, const unsigned long long* key, int* cnt, const int* off, int* localPoints, int cap,
                                                      int phase) {
	const int slot = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (slot >= s.nslots) return;
	const int r = rankOf[slot];
	const int n = r < 0 ? 0 : s.rowN[slot];
	int run = phase ? off[slot] : 0;
	const int* row = s.row(slot);
	for (int f0 = 0; f0 < n; f0 += 64) {
		const int f = f0 + lane;
		int p = -1;
		bool first = false;
		if (f < n) {
			p = row[f];
			first = p >= 0 && !s.ptBad[p] && key[p] == (((unsigned long long)r << 32) | (unsigned)f);
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

}  // namespace
}  // namespace mcs

using namespace mcs;

int covis_slots_of(const mcs_covis* h, const int64_t* ids, int n, int* out) {
	for (int i = 0; i < n; ++i)
		if ((out[i] = covis_slot(h, ids[i])) < 0) return fail(MCS_ERR_INVALID, "keyframe not in the store");
	return MCS_OK;
}

int check_point_ids(const mcs_covis* h, const int32_t* ids, int n, int lowest, bool distinct) {
	for (int i = 0; i < n; ++i)
		if (ids[i] < lowest || ids[i] >= h->maxPts)
			return fail(MCS_ERR_INVALID, lowest < 0 ? "map point id outside [-1, max_points)" : "map point id outside [0, max_points)");
	if (distinct) {
		std::vector<int32_t> v(ids, ids + n);
		std::sort(v.begin(), v.end());
		if (std::adjacent_find(v.begin(), v.end()) != v.end()) return fail(MCS_ERR_INVALID, "a map point is listed twice");
	}
	return MCS_OK;
}

int mcs_covis_create(mcs_ctx* c, int max_keyframes, int max_features, int max_points, mcs_covis** out) {
	if (!c || !out) return fail(MCS_ERR_INVALID, "null argument");
	if (max_keyframes < 1 || max_features < 1 || max_points < 1 || max_keyframes > (1 << 24) || max_features > (1 << 20))
		return fail(MCS_ERR_INVALID, "capacities must be >= 1 (keyframes <= 2^24, features <= 2^20)");
	HIPCHK(hipSetDevice(c->device));
	mcs_covis* h = new mcs_covis();
	h->ctx = c; h->maxKf = max_keyframes; h->maxFeat = max_features; h->maxPts = max_points;
	h->pitch = (max_features + 3) / 4 * 4;   // rows start 16-byte aligned
	h->wide = max_keyframes >= 65536;
	const size_t K = (size_t)max_keyframes, P = (size_t)max_points, rowBytes = K * h->pitch * 4;
	Layout lay;
	lay.piece(&h->rows, rowBytes); lay.piece(&h->drows, rowBytes); lay.piece(&h->dRowN, K * 4); lay.piece(&h->dLive, K); lay.piece(&h->dKfBad, K);
	lay.piece(&h->dIds, K * 8); lay.piece(&h->dT, K * 24); lay.piece(&h->ptBad, P); lay.piece(&h->mult, P * 4); lay.piece(&h->key, P * 8);
	lay.piece(&h->count, K * 4); lay.piece(&h->cnt, K * 4); lay.piece(&h->off, K * 4); lay.piece(&h->rankOf, K * 4);
	lay.piece(&h->octs, K * h->pitch); lay.piece(&h->obs, P * MCS_MAX_LEVELS * (h->wide ? 4 : 2)); lay.piece(&h->list, K * 4);
	const hipError_t e = h->mem.reserve(lay.total);
	if (e != hipSuccess) { delete h; return fail(MCS_ERR_HIP, std::string("covisibility store allocation failed: ") + hipGetErrorString(e)); }
	lay.place(h->mem.p);
	hipError_t e2 = hipMemsetAsync(h->mem.p, 0, lay.total, c->stream);
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
	h->id.clear(); h->live.clear(); h->rowN.clear(); h->slotOf.clear(); h->hasDesc.clear(); h->nLive = 0;
	return MCS_OK;
}

int mcs_covis_size(const mcs_covis* h, int* n) {
	if (!h || !n) return fail(MCS_ERR_INVALID, "null argument");
	*n = h->nLive;
	return MCS_OK;
}

int mcs_covis_slots(const mcs_covis* h, int* n) {
	if (!h || !n) return fail(MCS_ERR_INVALID, "null argument");
	*n = h->slots();
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
		if (h->slots() >= h->maxKf) return fail(MCS_ERR_CAPACITY, "more keyframes than the store's max_keyframes");
	}
	if (kind == MCS_MEM_HOST)
		if (int r = check_point_ids(h, points, n, -1, false)) return r;
	mcs_ctx* c = h->ctx;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	Staging st(c, kind == MCS_MEM_HOST);
	const int* src = nullptr;
	st.in(&src, points, (size_t)n * 4);
	if (int r = st.commit()) return r;
	const bool isNew = slot < 0;
	const bool keepOctaves = !isNew && h->rowN[slot] == n;
	if (isNew) {
		slot = h->slots();
		h->id.push_back(mnId); h->live.push_back(1); h->rowN.push_back(n); h->hasDesc.push_back(0); h->slotOf[mnId] = slot; ++h->nLive;
	} else h->rowN[slot] = n;
	if (!keepOctaves) h->hasDesc[slot] = 0;   // the descriptors go the way of the octaves
	if (!keepOctaves) HIPCHK(hipMemsetAsync(h->octs + h->at(slot), 0, (size_t)h->pitch, s));   // level 0 until mcs_covis_set_keyframe_octaves
	int* row = h->rows + h->at(slot);
	int* drow = h->drows + h->at(slot);
	const unsigned gp = blocks(h->pitch);
	hipLaunchKernelGGL(k_covis_set_row, dim3(gp), dim3(256), 0, s, src, n, h->maxPts, h->pitch, row);
	if (n > 0) hipLaunchKernelGGL(k_covis_first_index, dim3(blocks(n)), dim3(256), 0, s, row, n, h->key);
	hipLaunchKernelGGL(k_covis_distinct, dim3(gp), dim3(256), 0, s, row, n, h->pitch, h->key, drow);
	if (n > 0) hipLaunchKernelGGL(k_covis_reset_row_keys, dim3(blocks(n)), dim3(256), 0, s, row, n, h->key);
	hipLaunchKernelGGL(k_covis_meta, dim3(1), dim3(1), 0, s, slot, n, 1, 0, (long long)mnId, isNew ? 7 : 1, h->dRowN, h->dLive, h->dKfBad, h->dIds, h->dT);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_covis_set_keyframe_pose(mcs_covis* h, int n, const int64_t* mnIds, const double* t, mcs_mem_kind kind) {
	if (!h || n < 0 || (n > 0 && (!mnIds || !t))) return fail(MCS_ERR_INVALID, "null argument");
	std::vector<int> slots(n);
	if (int r = covis_slots_of(h, mnIds, n, slots.data())) return r;
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
	int slot;
	if (int r = covis_slots_of(h, &mnId, 1, &slot)) return r;
	HIPCHK(hipSetDevice(h->ctx->device));
	hipLaunchKernelGGL(k_covis_meta, dim3(1), dim3(1), 0, h->ctx->stream, slot, 0, 0, 0, 0ll, 1, h->dRowN, h->dLive, h->dKfBad, h->dIds, h->dT);
	HIPCHK(hipGetLastError());
	h->live[slot] = 0; h->rowN[slot] = 0; h->hasDesc[slot] = 0; --h->nLive;
	return MCS_OK;
}

int mcs_covis_set_keyframe_bad(mcs_covis* h, int64_t mnId, int bad) {
	if (!h) return fail(MCS_ERR_INVALID, "null argument");
	int slot;
	if (int r = covis_slots_of(h, &mnId, 1, &slot)) return r;
	HIPCHK(hipSetDevice(h->ctx->device));
	hipLaunchKernelGGL(k_covis_meta, dim3(1), dim3(1), 0, h->ctx->stream, slot, 0, 0, bad ? 1 : 0, 0ll, 2, h->dRowN, h->dLive, h->dKfBad, h->dIds, h->dT);
	HIPCHK(hipGetLastError());
	return MCS_OK;
}

int mcs_covis_set_points_bad(mcs_covis* h, const int32_t* ids, int n, const uint8_t* bad, mcs_mem_kind kind) {
	if (!h || n < 0 || (n > 0 && (!ids || !bad))) return fail(MCS_ERR_INVALID, "null argument");
	if (n == 0) return MCS_OK;
	if (kind == MCS_MEM_HOST)
		if (int r = check_point_ids(h, ids, n, 0, false)) return r;
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
	if (n > 0) hipLaunchKernelGGL(k_covis_mark, dim3(blocks(n)), dim3(256), 0, s, voter, n, h->maxPts, h->ptBad, h->mult, nullBad);
	if (S > 0) {
		h->ctx->tic("covis_count");
		hipLaunchKernelGGL(k_covis_count, dim3(blocks((long long)S * 64)), dim3(256), 0, s, h->view(S), h->mult, self, count);
		h->ctx->toc("covis_count");
	}
	if (n > 0) hipLaunchKernelGGL(k_covis_unmark, dim3(blocks(n)), dim3(256), 0, s, voter, n, h->maxPts, h->mult);
}

int mcs_covis_update_reference(mcs_covis* h, int32_t* frame_points, int nf, const double* frame_t, int cap, mcs_mem_kind kind, int64_t* local_kfs,
                               int32_t* local_weights, double* local_dist, int32_t* n_local, int64_t* ref_kf, int32_t* local_points, int32_t* n_points) {
	if (!h || !frame_t || !n_local || !ref_kf || !n_points || (nf > 0 && !frame_points) || (cap > 0 && !local_points)) return fail(MCS_ERR_INVALID, "null argument");
	if (nf < 0 || cap < 0) return fail(MCS_ERR_INVALID, "bad sizes");
	const int S = h->slots();
	if (S > 0 && (!local_kfs || !local_weights || !local_dist)) return fail(MCS_ERR_INVALID, "null argument");
	mcs_ctx* c = h->ctx;
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the local map is built in order: switch deferred searches off (mcs_ctx_set_async_search)");
	if (kind == MCS_MEM_HOST)
		if (int r = check_point_ids(h, frame_points, nf, -1, false)) return r;
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
	const CovisView v = h->view(S);
	const dim3 gf((unsigned)std::max(S, 1), blocks(h->pitch)), gw(blocks((long long)S * 64)), tb(256);
	covis_vote(h, fp, nf, 1, -1, S, h->count, s);
	hipLaunchKernelGGL(k_covis_local, dim3(1), dim3(1024), 0, s, v, h->count, ft, oKfs, oW, oD, oNl, oRef, h->rankOf);
	if (cap > 0) HIPCHK(hipMemsetAsync(oLp, 0xFF, (size_t)cap * 4, s));
	if (S > 0) {
		hipLaunchKernelGGL(k_covis_first, gf, tb, 0, s, v, h->rankOf, h->key, 0);
		hipLaunchKernelGGL(k_covis_emit, gw, tb, 0, s, v, h->rankOf, h->key, h->cnt, h->off, oLp, cap, 0);
	}
	hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(1024), 0, s, h->cnt, S, h->off, oNp);
	if (S > 0) {
		hipLaunchKernelGGL(k_covis_emit, gw, tb, 0, s, v, h->rankOf, h->key, h->cnt, h->off, oLp, cap, 1);
		hipLaunchKernelGGL(k_covis_first, gf, tb, 0, s, v, h->rankOf, h->key, 1);
	}
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_covis_update_connections(mcs_covis* h, int nq, const int64_t* mnIds, mcs_mem_kind kind, int32_t* count, int32_t* n_counted, int64_t* ordered,
                                 int32_t* ordered_w, int32_t* n_ordered) {
	if (!h || nq < 0 || (nq > 0 && (!mnIds || !count || !n_counted || !ordered || !ordered_w || !n_ordered))) return fail(MCS_ERR_INVALID, "null argument");
	mcs_ctx* c = h->ctx;
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the covisibility counts run in order: switch deferred searches off (mcs_ctx_set_async_search)");
	const int S = h->slots();
	std::vector<int> slots(nq);
	if (int r = covis_slots_of(h, mnIds, nq, slots.data())) return r;
	if (nq == 0) return MCS_OK;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	Staging st(c, kind == MCS_MEM_HOST);
	int* oC = nullptr; int* oN = nullptr; long long* oO = nullptr; int* oW = nullptr; int* oNo = nullptr;
	const size_t QS = (size_t)nq * S;
	st.out(&oC, count, QS * 4); st.out(&oN, n_counted, (size_t)nq * 4); st.out(&oO, ordered, QS * 8); st.out(&oW, ordered_w, QS * 4); st.out(&oNo, n_ordered, (size_t)nq * 4);
	if (int r = st.commit()) return r;
	for (int q = 0; q < nq; ++q)   // the rows do not change: a batch equals the sequence
		covis_vote(h, h->rows + h->at(slots[q]), h->rowN[slots[q]], 0, slots[q], S, oC + (size_t)q * S, s);
	hipLaunchKernelGGL(k_covis_order, dim3(nq), dim3(1024), 0, s, oC, h->dIds, S, 30, oN, oO, oW, oNo);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}
