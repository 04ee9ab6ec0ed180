// mcs_covis.hip — the local map and the covisibility counts on the device:
//   cTracking::UpdateReferenceKeyFrames / UpdateReferencePoints   src/cTracking.cpp:1024-1123   (mcs_covis_update_reference)
//   cMultiKeyFrame::UpdateConnections (counting and ordering)      src/cMultiKeyFrame.cpp:406-500 (mcs_covis_update_connections)
//   cLocalMapping::KeyFrameCulling / MapPointCulling                src/cLocalMapping.cpp:517-593, 187-221 (mcs_covis_cull_keyframes / _cull_points; below)
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

// ---- KeyFrameCulling / MapPointCulling
// obs[p][level] = the live keyframes whose FIRST entry of point p (the distinct row's) lies at that octave: MCS_MAX_LEVELS counters per point, 16 bits each
// packed two to a word while the store has fewer than 65 536 slots (WIDE = false), 32 bits otherwise.  Observations() is the sum of a point's counters.  The
// table is zero between calls: a call marks the points it asks about (mult), counts those, and clears exactly those again.
static_assert(MCS_MAX_LEVELS == 16, "the counter rows below are written for 16 levels");
constexpr int kListSlot = (1 << 24) - 1, kListNotErase = 1 << 29, kListSkip = 1 << 30;   // a list entry: slot | flags (max_keyframes <= 2^24)

template <bool WIDE>
__device__ __forceinline__ void obs_atomic_inc(uint32_t* obs, int p, unsigned lvl) {
	if (WIDE) atomicAdd(&obs[(size_t)p * 16 + lvl], 1u);
	else atomicAdd(&obs[(size_t)p * 8 + (lvl >> 1)], 1u << ((lvl & 1) * 16));
}
// d = +1 / -1 by the ONE thread that owns point p in this phase; a counter that is decremented was counted before, so no borrow crosses into its neighbour
template <bool WIDE>
__device__ __forceinline__ void obs_add(uint32_t* obs, int p, unsigned lvl, int d) {
	if (WIDE) obs[(size_t)p * 16 + lvl] += (uint32_t)d;
	else obs[(size_t)p * 8 + (lvl >> 1)] += (uint32_t)d << ((lvl & 1) * 16);
}
template <bool WIDE>
__device__ __forceinline__ void obs_zero(uint32_t* obs, int p) {
	uint4* r = reinterpret_cast<uint4*>(obs + (size_t)p * (WIDE ? 16 : 8));
	const uint4 z = make_uint4(0, 0, 0, 0);
	r[0] = z; r[1] = z;
	if (WIDE) { r[2] = z; r[3] = z; }
}
// all = every counter of point p, pre = the counters of levels 0 .. top.  The row is read with 16-byte loads and stays in registers (no private array).
template <bool WIDE>
__device__ __forceinline__ void obs_sums(const uint32_t* obs, int p, int top, int& all, int& pre) {
	int a = 0, s = 0;
	const uint4* r = reinterpret_cast<const uint4*>(obs + (size_t)p * (WIDE ? 16 : 8));
	if (WIDE) {
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const uint4 v = r[q];
			a += (int)(v.x + v.y + v.z + v.w);
			s += (4 * q <= top ? (int)v.x : 0) + (4 * q + 1 <= top ? (int)v.y : 0) + (4 * q + 2 <= top ? (int)v.z : 0) + (4 * q + 3 <= top ? (int)v.w : 0);
		}
	} else {
#pragma unroll
		for (int q = 0; q < 2; ++q) {
			const uint4 v = r[q];
			const uint32_t w[4] = {v.x, v.y, v.z, v.w};   // constant indices after unrolling
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const int lo = (int)(w[j] & 0xFFFFu), hi = (int)(w[j] >> 16), l = 8 * q + 2 * j;
				a += lo + hi;
				s += (l <= top ? lo : 0) + (l + 1 <= top ? hi : 0);
			}
		}
	}
	all = a; pre = s;
}

__global__ __launch_bounds__(256) void k_cull_set_octaves(const uint8_t* src, int n, int pitch, uint8_t* oct) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= pitch) return;
	const uint8_t v = i < n ? src[i] : 0;
	oct[i] = v >= MCS_MAX_LEVELS ? (uint8_t)(MCS_MAX_LEVELS - 1) : v;
}
struct ListChunk { int v[128]; int n; };
__global__ void k_cull_put_list(ListChunk c, int* list) {
	if ((int)threadIdx.x < c.n) list[threadIdx.x] = c.v[threadIdx.x];
}
// the points of the listed keyframes: grid (listed keyframe, 256 features)
__global__ __launch_bounds__(256) void k_cull_mark_rows(const int* list, const int* drows, int pitch, const int* rowN, int* mult) {
	const int slot = list[blockIdx.x] & kListSlot, f = blockIdx.y * 256 + threadIdx.x;
	if (f >= rowN[slot]) return;
	const int p = drows[(size_t)slot * pitch + f];
	if (p >= 0) mult[p] = 1;
}
template <bool WIDE>
__global__ __launch_bounds__(256) void k_cull_unmark_rows(const int* list, const int* drows, int pitch, const int* rowN, int* mult, uint32_t* obs) {
	const int slot = list[blockIdx.x] & kListSlot, f = blockIdx.y * 256 + threadIdx.x;
	if (f >= rowN[slot]) return;
	const int p = drows[(size_t)slot * pitch + f];
	if (p >= 0) { mult[p] = 0; obs_zero<WIDE>(obs, p); }
}
// The wide pass: one wave per slot, the walk of k_covis_count with the octave row alongside (one 4-byte load per 16-byte load of ids); every entry that names
// a marked point adds one to that point's counter of the entry's level.  Bad keyframes observe (the reference has no test there), erased slots do not.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_cull_observe(const int* __restrict__ drows, const uint8_t* __restrict__ octs, int pitch, const int* __restrict__ rowN,
                                                       const uint8_t* __restrict__ live, const int* __restrict__ mult, int nslots, uint32_t* __restrict__ obs) {
	const int slot = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (slot >= nslots || !live[slot]) return;
	const int n4 = (rowN[slot] + 3) >> 2;
	const int4* r = reinterpret_cast<const int4*>(drows + (size_t)slot * pitch);
	const uint32_t* o = reinterpret_cast<const uint32_t*>(octs + (size_t)slot * pitch);
	for (int j = lane; j < n4; j += 64) {
		const int4 v = r[j];
		const uint32_t l = o[j];
		if (v.x >= 0 && mult[v.x]) obs_atomic_inc<WIDE>(obs, v.x, l & 0xFFu);
		if (v.y >= 0 && mult[v.y]) obs_atomic_inc<WIDE>(obs, v.y, (l >> 8) & 0xFFu);
		if (v.z >= 0 && mult[v.z]) obs_atomic_inc<WIDE>(obs, v.z, (l >> 16) & 0xFFu);
		if (v.w >= 0 && mult[v.w]) obs_atomic_inc<WIDE>(obs, v.w, l >> 24);
	}
}
// The serial chain (src/cLocalMapping.cpp:527-591): ONE workgroup judges the listed keyframes one after another, because a culled keyframe changes what the
// next one sees.  Per keyframe: (1) take its own observations out of the table (:561-562, pKF never counts; the distinct row holds each point once, at its
// first level); (2) per feature of the full row: nMPs, Observations() - 1 >= 3, nObs = the counters up to octave + 1 >= 5 (:538-587); (3) decide (:589);
// (4) culled: the observations stay out, every point left with two or fewer observers goes bad and is emitted in feature order
// (src/cMultiKeyFrame.cpp:591-593, src/cMapPoint.cpp:96-116, 185-204) — otherwise put the observations back.  The table, ptBad and the outputs are touched by
// this workgroup alone; a barrier with a workgroup fence separates the phases.  A point that went bad is skipped by every later keyframe through ptBad, which
// is what nulling its entries does in the reference.
template <bool WIDE>
__global__ __launch_bounds__(1024) void k_cull_chain(const int* __restrict__ list, int n, const int* __restrict__ rows, const int* __restrict__ drows,
                                                      const uint8_t* __restrict__ octs, int pitch, const int* __restrict__ rowN, uint8_t* ptBad, uint8_t* kfBad,
                                                      uint32_t* obs, int cap, int* verdict, int* nMps, int* nRed, int* badPoints, int* nBad) {
	__shared__ int wM[16], wR[16], wE[16];
	__shared__ int base;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	if (tid == 0) base = 0;
	__syncthreads();
	for (int k = 0; k < n; ++k) {
		const int e = list[k], slot = e & kListSlot;
		if (e & kListSkip) {   // :531
			if (tid == 0) { verdict[k] = 3; nMps[k] = 0; nRed[k] = 0; }
			continue;
		}
		const int nrow = rowN[slot];
		const int* row = rows + (size_t)slot * pitch;
		const int* drow = drows + (size_t)slot * pitch;
		const uint8_t* oct = octs + (size_t)slot * pitch;
		for (int i = tid; i < nrow; i += 1024) {
			const int p = drow[i];
			if (p >= 0) obs_add<WIDE>(obs, p, oct[i], -1);
		}
		__threadfence_block();
		__syncthreads();
		int nm = 0, nr = 0;
		for (int i = tid; i < nrow; i += 1024) {
			const int p = row[i];
			if (p < 0 || ptBad[p]) continue;   // :541-543
			++nm;                                // :545
			const int lv = oct[i];             // :551
			int all, pre;
			obs_sums<WIDE>(obs, p, lv + 1 < MCS_MAX_LEVELS ? lv + 1 : MCS_MAX_LEVELS - 1, all, pre);
			if (all + 1 > 3 && pre >= 5) ++nr;   // :548, :572-583
		}
		nm = wave_sum(nm); nr = wave_sum(nr);
		if (lane == 0) { wM[w] = nm; wR[w] = nr; }
		__syncthreads();
		nm = 0; nr = 0;
		for (int j = 0; j < 16; ++j) { nm += wM[j]; nr += wR[j]; }
		const bool redundant = (double)nr > 0.9 * (double)nm;   // :589
		const bool cull = redundant && !(e & kListNotErase);   // src/cMultiKeyFrame.cpp:580-584
		if (tid == 0) {
			verdict[k] = redundant ? (cull ? 1 : 2) : 0; nMps[k] = nm; nRed[k] = nr;
			if (cull) kfBad[slot] = 1;
		}
		if (cull) {
			for (int i0 = 0; i0 < nrow; i0 += 1024) {
				const int i = i0 + tid;
				const int p = i < nrow ? drow[i] : -1;
				bool goes = false;
				if (p >= 0 && !ptBad[p]) {
					int all, pre;
					obs_sums<WIDE>(obs, p, MCS_MAX_LEVELS - 1, all, pre);
					goes = all <= 2;   // src/cMapPoint.cpp:109
				}
				const unsigned long long b = __ballot(goes);
				if (lane == 0) wE[w] = __popcll(b);
				__syncthreads();
				int rank = base + __popcll(b & lanes_below());
				for (int j = 0; j < w; ++j) rank += wE[j];
				if (goes) {
					ptBad[p] = 1;
					if (rank < cap) badPoints[rank] = p;
				}
				__syncthreads();
				if (tid == 0) { int t = 0; for (int j = 0; j < 16; ++j) t += wE[j]; base += t; }
				__syncthreads();
			}
		} else {
			for (int i = tid; i < nrow; i += 1024) {
				const int p = drow[i];
				if (p >= 0) obs_add<WIDE>(obs, p, oct[i], 1);
			}
		}
		__threadfence_block();
		__syncthreads();
	}
	if (tid == 0) *nBad = base;
}

// ---- the listed points (mcs_covis_observations, mcs_covis_cull_points): key[p] = the first entry that names p
__global__ __launch_bounds__(256) void k_cull_pt_mark(const int* ids, int n, int maxPoints, int* mult, unsigned long long* key) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = ids[i];
	if ((unsigned)p >= (unsigned)maxPoints) return;
	mult[p] = 1;
	if (key) atomicMin(&key[p], (unsigned long long)i);
}
template <bool WIDE>
__global__ __launch_bounds__(256) void k_cull_pt_obs(const int* ids, int n, int maxPoints, const uint8_t* ptBad, const uint32_t* obs, int* nobs) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = ids[i];
	int all = 0, pre = 0;
	if ((unsigned)p < (unsigned)maxPoints && !ptBad[p]) obs_sums<WIDE>(obs, p, 0, all, pre);   // a bad point has no observations (src/cMapPoint.cpp:193)
	nobs[i] = all;
}
template <bool WIDE>
__global__ __launch_bounds__(256) void k_cull_pt_verdict(unsigned long long cur, const int* ids, int n, const int* found, const int* visible, const long long* firstKf,
                                                          int maxPoints, const uint8_t* ptBad, const unsigned long long* key, const uint32_t* obs, int* verdict) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = ids[i];
	int r = 1;
	if ((unsigned)p < (unsigned)maxPoints && !ptBad[p]) {   // :195
		const int j = (int)key[p];
		int all, pre;
		obs_sums<WIDE>(obs, p, 0, all, pre);
		const unsigned long long d = cur - (unsigned long long)firstKf[j];   // unsigned long - long
		if ((double)found[j] / (double)visible[j] < 0.25) r = 2;            // :200, cMapPoint::GetFoundRatio
		else if (d >= 2 && all <= 2) r = 3;                                  // :206-207
		else if (d >= 3) r = 4;                                              // :213
		else r = 0;
	}
	verdict[i] = r;
}
template <bool WIDE>
__global__ __launch_bounds__(256) void k_cull_pt_unmark(const int* ids, int n, int maxPoints, const int* verdict, uint8_t* ptBad, int* mult, unsigned long long* key,
                                                         uint32_t* obs) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = ids[i];
	if ((unsigned)p >= (unsigned)maxPoints) return;
	if (verdict && (verdict[i] == 2 || verdict[i] == 3)) ptBad[p] = 1;   // cMapPoint::SetBadFlag
	mult[p] = 0;
	if (key) key[p] = kNoKey;
	obs_zero<WIDE>(obs, p);
}

// ---- cMapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors for a list of points (mcs_covis_update_points)
// mult[p] = 1 + the LAST list index that names p (atomicMax: any order gives the same): that entry owns the point's segment, every copy reads it.
// A segment = the (slot << 32 | feature) entries of every live row that name the point, sorted: ascending slot, ascending feature within a slot.
__global__ __launch_bounds__(256) void k_mp_mark(const int* ids, int n, int maxPoints, int* mult) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = ids[i];
	if ((unsigned)p < (unsigned)maxPoints) atomicMax(&mult[p], i + 1);
}
__global__ __launch_bounds__(256) void k_mp_set_desc(const uint32_t* src, int n, int srcWords, int dimWords, uint32_t* dst) {
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
	if (t >= (long long)n * dimWords) return;
	const long long r = t / dimWords;
	dst[t] = src[r * srcWords + (t - r * dimWords)];
}
// The walk of k_covis_count over the FULL rows (every feature of a keyframe that holds the point is an entry).  FILL = false: seg[j] = entries of listed
// point j; FILL = true: each entry takes the next free place of its segment (seg = the cursors, zero at the start) — the order inside a segment is whatever
// the atomics gave, k_mp_sort makes it a function of the store.
template <bool FILL>
__global__ __launch_bounds__(256) void k_mp_stream(const int* __restrict__ rows, int pitch, const int* __restrict__ rowN, const uint8_t* __restrict__ live,
                                                    const int* __restrict__ mult, int nslots, int* seg, const int* __restrict__ off, unsigned long long* ent) {
	const int slot = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (slot >= nslots || !live[slot]) return;
	const int n4 = (rowN[slot] + 3) >> 2;
	const int4* r = reinterpret_cast<const int4*>(rows + (size_t)slot * pitch);
	for (int j = lane; j < n4; j += 64) {
		const int4 v = r[j];
		const int pv[4] = {v.x, v.y, v.z, v.w};   // constant indices after unrolling
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			if (pv[q] < 0) continue;
			const int m = mult[pv[q]];
			if (!m) continue;
			if (FILL) ent[off[m - 1] + atomicAdd(&seg[m - 1], 1)] = ((unsigned long long)slot << 32) | (unsigned)(4 * j + q);
			else atomicAdd(&seg[m - 1], 1);
		}
	}
}
// one workgroup per listed point: rank by counting (the keys of a segment are distinct), 256 keys at a time through LDS
__global__ __launch_bounds__(256) void k_mp_sort(const int* __restrict__ off, const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out) {
	__shared__ unsigned long long tile[256];
	const int lo = off[blockIdx.x], L = off[blockIdx.x + 1] - lo, tid = threadIdx.x;
	for (int e0 = 0; e0 < L; e0 += 256) {
		const int e = e0 + tid;
		const unsigned long long key = e < L ? in[lo + e] : 0ull;
		int rank = 0;
		for (int x0 = 0; x0 < L; x0 += 256) {
			__syncthreads();
			tile[tid] = x0 + tid < L ? in[lo + x0 + tid] : ~0ull;
			__syncthreads();
			const int m = min(256, L - x0);
			for (int x = 0; x < m; ++x) rank += tile[x] < key ? 1 : 0;
		}
		if (e < L) out[lo + rank] = key;
	}
}
// One wave per listed point: status, level, normal and depth range (src/cMapPoint.cpp:449-492).  The unit vectors of 64 entries are formed in parallel; the
// additions are ONE chain in segment order (every lane runs it on the shuffled terms), so the sum is the reference's whatever the machine does.
// cv::norm = sqrt(((0 + x^2) + y^2) + z^2); Vec / double and Vec / int multiply by 1. / alpha.
__global__ __launch_bounds__(256) void k_mp_normal(const int* __restrict__ ids, int n, int maxPoints, const uint8_t* __restrict__ ptBad, const int* __restrict__ mult,
                                                    const int* __restrict__ off, const unsigned long long* __restrict__ ent, const double* __restrict__ pos,
                                                    const long long* __restrict__ refKf, const long long* __restrict__ kfIds, const uint8_t* __restrict__ live,
                                                    int nslots, const double* __restrict__ kt, const uint8_t* __restrict__ octs, int pitch,
                                                    const double* __restrict__ sf, int nlevels, int* st, double* normal, double* minD, double* maxD, double* minI,
                                                    double* maxI, int* status) {
	const int i = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (i >= n) return;
	const int p = ids[i];
	int code = 0, ref = -1, level = 1, lo = 0, hi = 0;   // :479
	if ((unsigned)p >= (unsigned)maxPoints || ptBad[p]) code = 1;   // :457
	else {
		const long long want = refKf[i];
		int a = 0, b = nslots;
		while (a < b) { const int m = (a + b) >> 1; if (kfIds[m] < want) a = m + 1; else b = m; }   // slot order is id order
		if (a < nslots && kfIds[a] == want && live[a]) ref = a; else code = 2;
	}
	if (code == 0) {
		const int r = mult[p] - 1;
		lo = off[r]; hi = off[r + 1];
		for (int c = lo; c < hi; c += 64) {   // observations[pRefKF][0]: the first entry of the reference keyframe's slot (:480-481)
			const int idx = c + lane;
			const unsigned long long e = idx < hi ? ent[idx] : ~0ull;
			const unsigned long long hit = __ballot(idx < hi && (int)(e >> 32) == ref);
			if (hit) {
				const int feat = __shfl((int)(e & 0xFFFFFFFFull), __ffsll((long long)hit) - 1);
				level = octs[(size_t)ref * pitch + feat];
				break;
			}
		}
		if (level >= nlevels) code = 3;   // mvScaleFactors[level] out of bounds
	}
	if (lane == 0) { st[i] = code; if (status) status[i] = code; }
	if (code) return;
	const double px = pos[3 * i], py = pos[3 * i + 1], pz = pos[3 * i + 2];
	double sx = 0.0, sy = 0.0, sz = 0.0;
	int nobs = 0;
	for (int c = lo; c < hi; c += 64) {   // :466-474: one term per observing keyframe = per distinct slot of the segment
		const int idx = c + lane;
		bool head = false;
		double tx = 0.0, ty = 0.0, tz = 0.0;
		if (idx < hi) {
			const int slot = (int)(ent[idx] >> 32);
			head = idx == lo || (int)(ent[idx - 1] >> 32) != slot;
			if (head) {
				const double dx = px - kt[3 * slot], dy = py - kt[3 * slot + 1], dz = pz - kt[3 * slot + 2];
				double s = 0.0;
				s += dx * dx; s += dy * dy; s += dz * dz;
				const double inv = 1.0 / sqrt(s);
				tx = dx * inv; ty = dy * inv; tz = dz * inv;
			}
		}
		unsigned long long b = __ballot(head);
		nobs += __popcll(b);
		while (b) {
			const int l = __ffsll((long long)b) - 1;
			b &= b - 1;
			sx += __shfl(tx, l); sy += __shfl(ty, l); sz += __shfl(tz, l);
		}
	}
	if (lane) return;
	const double dx = px - kt[3 * ref], dy = py - kt[3 * ref + 1], dz = pz - kt[3 * ref + 2];   // :476-477
	double s = 0.0;
	s += dx * dx; s += dy * dy; s += dz * dz;
	const double dist = sqrt(s), f = sf[level];
	const double mn = ((1.0 / f) * dist) / f, mx = (f * dist) * sf[nlevels - 1 - level];   // :488-489
	const double in = 1.0 / (double)nobs;                                               // :490
	if (normal) { normal[3 * i] = sx * in; normal[3 * i + 1] = sy * in; normal[3 * i + 2] = sz * in; }
	if (minD) minD[i] = mn;
	if (maxD) maxD[i] = mx;
	if (minI) minI[i] = 0.8 * mn;   // GetMinDistanceInvariance / GetMaxDistanceInvariance
	if (maxI) maxI[i] = 1.2 * mx;
}
// One wave per listed point, for the entry that owns the segment of a point that is not bad: the entries of keyframes that are not bad (:319), in segment
// order.  phase 0: cntE[i] = their number; phase 1: from offE[i] on, the entries and a copy of their descriptor (and mask) rows — k_distinct's input.
__global__ __launch_bounds__(256) void k_mp_collect(const int* __restrict__ ids, int n, int maxPoints, const uint8_t* __restrict__ ptBad, const int* __restrict__ mult,
                                                     const int* __restrict__ off, const unsigned long long* __restrict__ ent, const uint8_t* __restrict__ kfBad,
                                                     int pitch, int dim, const uint8_t* __restrict__ slabD, const uint8_t* __restrict__ slabM, int* cntE,
                                                     const int* __restrict__ offE, unsigned long long* entE, uint8_t* rowsD, uint8_t* rowsM, int phase) {
	const int i = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (i >= n) return;
	const int p = ids[i];
	const bool own = (unsigned)p < (unsigned)maxPoints && !ptBad[p] && mult[p] - 1 == i;   // :304
	int run = phase ? offE[i] : 0;
	const int lo = own ? off[i] : 0, hi = own ? off[i + 1] : 0;
	for (int c = lo; c < hi; c += 64) {
		const int idx = c + lane;
		const unsigned long long e = idx < hi ? ent[idx] : 0ull;
		const bool take = idx < hi && !kfBad[(int)(e >> 32)];
		const unsigned long long b = __ballot(take);
		if (phase && take) {
			const size_t to = (size_t)(run + __popcll(b & lanes_below())), from = (size_t)(e >> 32) * pitch + (size_t)(e & 0xFFFFFFFFull);
			entE[to] = e;
			const uint4* s = reinterpret_cast<const uint4*>(slabD + from * dim);
			uint4* d = reinterpret_cast<uint4*>(rowsD + to * dim);
			for (int w = 0; w < dim / 16; ++w) d[w] = s[w];
			if (slabM) {
				const uint4* sm = reinterpret_cast<const uint4*>(slabM + from * dim);
				uint4* dm = reinterpret_cast<uint4*>(rowsM + to * dim);
				for (int w = 0; w < dim / 16; ++w) dm[w] = sm[w];
			}
		}
		run += __popcll(b);
	}
	if (!phase && lane == 0) cntE[i] = run;
}
// the winners (:382-387): entry i of status 0 reads the choice made for its point's segment
__global__ __launch_bounds__(256) void k_mp_winner(const int* __restrict__ ids, int n, const int* __restrict__ st, const int* __restrict__ mult,
                                                    const int* __restrict__ offE, const unsigned long long* __restrict__ entE, const int* __restrict__ bestIdx,
                                                    const long long* __restrict__ kfIds, int dim, const uint8_t* __restrict__ rowsD, const uint8_t* __restrict__ rowsM,
                                                    uint32_t* desc, uint32_t* mask, int* nDesc, long long* bestKf, int* bestFeat) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || st[i]) return;
	const int r = mult[ids[i]] - 1, N = offE[r + 1] - offE[r];
	if (nDesc) nDesc[i] = N;
	if (N <= 0) {   // :309-310, :332-333: the old descriptor stays
		if (bestKf) bestKf[i] = -1;
		if (bestFeat) bestFeat[i] = -1;
		return;
	}
	const size_t row = (size_t)offE[r] + bestIdx[r];
	const unsigned long long e = entE[row];
	if (bestKf) bestKf[i] = kfIds[(int)(e >> 32)];
	if (bestFeat) bestFeat[i] = (int)(e & 0xFFFFFFFFull);
	const int W = dim / 4;
	const uint32_t* s = reinterpret_cast<const uint32_t*>(rowsD + row * dim);
	for (int w = 0; w < W; ++w) desc[(size_t)i * W + w] = s[w];
	if (mask && rowsM) {
		const uint32_t* sm = reinterpret_cast<const uint32_t*>(rowsM + row * dim);
		for (int w = 0; w < W; ++w) mask[(size_t)i * W + w] = sm[w];
	}
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
	// culling: the octave rows (the slot layout of rows / drows), the per-point level counters (zero between calls) and the listed slots of one call
	uint8_t* octs = nullptr; uint32_t* obs = nullptr; int* list = nullptr;
	bool wide = false;   // 32-bit counters: a store of 65 536 slots or more
	// descriptors (mcs_covis_set_keyframe_descriptors): one slab of rows and one of masks in the slot layout of `rows`, allocated at the first call, which
	// also fixes the row width and whether masks exist; hasDesc = the host's view of which slots hold descriptors
	DevBuf descSlab, maskSlab;
	int descDim = 0; bool descMasks = false;
	std::vector<uint8_t> hasDesc;
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
	h->wide = max_keyframes >= 65536;
	const size_t oOct = cv.take(K * h->pitch), oObs = cv.take(P * MCS_MAX_LEVELS * (h->wide ? 4 : 2)), oList = cv.take(K * 4);
	const hipError_t e = h->mem.reserve(cv.total);
	if (e != hipSuccess) { delete h; return fail(MCS_ERR_HIP, std::string("covisibility store allocation failed: ") + hipGetErrorString(e)); }
	uint8_t* b = h->mem.p;
	h->rows = (int*)(b + oRows); h->drows = (int*)(b + oDrows); h->dRowN = (int*)(b + oN); h->dLive = b + oLive; h->dKfBad = b + oBad;
	h->dIds = (long long*)(b + oIds); h->dT = (double*)(b + oT); h->ptBad = b + oPt; h->mult = (int*)(b + oMult); h->key = (unsigned long long*)(b + oKey);
	h->count = (int*)(b + oCount); h->cnt = (int*)(b + oCnt); h->off = (int*)(b + oOff); h->rankOf = (int*)(b + oRank);
	h->octs = b + oOct; h->obs = (uint32_t*)(b + oObs); h->list = (int*)(b + oList);
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
	const bool keepOctaves = !isNew && h->rowN[slot] == n;
	if (isNew) {
		slot = (int)h->id.size();
		h->id.push_back(mnId); h->live.push_back(1); h->rowN.push_back(n); h->hasDesc.push_back(0); h->slotOf[mnId] = slot; ++h->nLive;
	} else h->rowN[slot] = n;
	if (!keepOctaves) h->hasDesc[slot] = 0;   // the descriptors go the way of the octaves
	if (!keepOctaves) HIPCHK(hipMemsetAsync(h->octs + (size_t)slot * h->pitch, 0, (size_t)h->pitch, s));   // level 0 until mcs_covis_set_keyframe_octaves
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
	h->live[slot] = 0; h->rowN[slot] = 0; h->hasDesc[slot] = 0; --h->nLive;
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

// ---- KeyFrameCulling / MapPointCulling
int mcs_covis_set_keyframe_octaves(mcs_covis* h, int64_t mnId, const uint8_t* octaves, int n, mcs_mem_kind kind) {
	if (!h || (n > 0 && !octaves)) return fail(MCS_ERR_INVALID, "null argument");
	const int slot = covis_slot(h, mnId);
	if (slot < 0) return fail(MCS_ERR_INVALID, "keyframe not in the store");
	if (n != h->rowN[slot]) return fail(MCS_ERR_INVALID, "one octave per feature of the keyframe's row");
	if (kind == MCS_MEM_HOST)
		for (int i = 0; i < n; ++i)
			if (octaves[i] >= MCS_MAX_LEVELS) return fail(MCS_ERR_INVALID, "octave outside [0, MCS_MAX_LEVELS)");
	mcs_ctx* c = h->ctx;
	HIPCHK(hipSetDevice(c->device));
	Staging st(c, kind == MCS_MEM_HOST);
	const uint8_t* src = nullptr;
	st.in(&src, octaves, (size_t)n);
	if (int r = st.commit()) return r;
	hipLaunchKernelGGL(k_cull_set_octaves, dim3(blocks(h->pitch)), dim3(256), 0, c->stream, src, n, h->pitch, h->octs + (size_t)slot * h->pitch);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

// the wide pass over every slot; the marked points' counters are complete behind it
static void cull_observe(mcs_covis* h, int S, hipStream_t s) {
	if (S <= 0) return;
	h->ctx->tic("cull_observe");
	const dim3 g(blocks((long long)S * 64)), b(256);
	if (h->wide) hipLaunchKernelGGL(k_cull_observe<true>, g, b, 0, s, (const int*)h->drows, (const uint8_t*)h->octs, h->pitch, (const int*)h->dRowN, (const uint8_t*)h->dLive, (const int*)h->mult, S, h->obs);
	else hipLaunchKernelGGL(k_cull_observe<false>, g, b, 0, s, (const int*)h->drows, (const uint8_t*)h->octs, h->pitch, (const int*)h->dRowN, (const uint8_t*)h->dLive, (const int*)h->mult, S, h->obs);
	h->ctx->toc("cull_observe");
}

int mcs_covis_cull_keyframes(mcs_covis* h, int n, const int64_t* mnIds, const uint8_t* not_erase, int cap, mcs_mem_kind kind, int32_t* verdict, int32_t* n_mps,
                             int32_t* n_redundant, int32_t* bad_points, int32_t* n_bad_points) {
	if (!h || !n_bad_points || n < 0 || cap < 0 || (n > 0 && (!mnIds || !verdict || !n_mps || !n_redundant)) || (cap > 0 && !bad_points))
		return fail(MCS_ERR_INVALID, "null argument / bad sizes");
	mcs_ctx* c = h->ctx;
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "keyframes are culled in order: switch deferred searches off (mcs_ctx_set_async_search)");
	const int S = (int)h->id.size();
	std::vector<int> list(n);
	std::vector<uint8_t> seen(S, 0);
	int maxRow = 0;
	for (int k = 0; k < n; ++k) {
		const int slot = covis_slot(h, mnIds[k]);
		if (slot < 0) return fail(MCS_ERR_INVALID, "keyframe not in the store");
		if (seen[slot]) return fail(MCS_ERR_INVALID, "a keyframe is listed twice");
		seen[slot] = 1;
		list[k] = slot | (mnIds[k] == 0 ? kListSkip : 0) | (not_erase && not_erase[k] ? kListNotErase : 0);
		maxRow = std::max(maxRow, h->rowN[slot]);
	}
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	Staging st(c, kind == MCS_MEM_HOST);
	int* oV = nullptr; int* oM = nullptr; int* oR = nullptr; int* oB = nullptr; int* oNb = nullptr;
	st.out(&oV, verdict, (size_t)n * 4); st.out(&oM, n_mps, (size_t)n * 4); st.out(&oR, n_redundant, (size_t)n * 4); st.out(&oB, bad_points, (size_t)cap * 4);
	st.out(&oNb, n_bad_points, 4);
	if (int r = st.commit()) return r;
	// the list travels in the arguments of small launches, 128 slots at a time: no copy from host memory that the call would have to outwait
	for (int k0 = 0; k0 < n; k0 += 128) {
		ListChunk ch;
		ch.n = std::min(128, n - k0);
		for (int k = 0; k < 128; ++k) ch.v[k] = k < ch.n ? list[k0 + k] : 0;
		hipLaunchKernelGGL(k_cull_put_list, dim3(1), dim3(128), 0, s, ch, h->list + k0);
	}
	if (cap > 0) HIPCHK(hipMemsetAsync(oB, 0xFF, (size_t)cap * 4, s));
	const dim3 gl((unsigned)std::max(n, 1), blocks(std::max(maxRow, 1)));
	const bool rowsToMark = n > 0 && maxRow > 0;
	if (rowsToMark) {
		hipLaunchKernelGGL(k_cull_mark_rows, gl, dim3(256), 0, s, (const int*)h->list, (const int*)h->drows, h->pitch, (const int*)h->dRowN, h->mult);
		cull_observe(h, S, s);
	}
	c->tic("cull_chain");
	if (h->wide) hipLaunchKernelGGL(k_cull_chain<true>, dim3(1), dim3(1024), 0, s, (const int*)h->list, n, (const int*)h->rows, (const int*)h->drows, (const uint8_t*)h->octs, h->pitch, (const int*)h->dRowN, h->ptBad, h->dKfBad, h->obs, cap, oV, oM, oR, oB, oNb);
	else hipLaunchKernelGGL(k_cull_chain<false>, dim3(1), dim3(1024), 0, s, (const int*)h->list, n, (const int*)h->rows, (const int*)h->drows, (const uint8_t*)h->octs, h->pitch, (const int*)h->dRowN, h->ptBad, h->dKfBad, h->obs, cap, oV, oM, oR, oB, oNb);
	c->toc("cull_chain");
	if (rowsToMark) {
		if (h->wide) hipLaunchKernelGGL(k_cull_unmark_rows<true>, gl, dim3(256), 0, s, (const int*)h->list, (const int*)h->drows, h->pitch, (const int*)h->dRowN, h->mult, h->obs);
		else hipLaunchKernelGGL(k_cull_unmark_rows<false>, gl, dim3(256), 0, s, (const int*)h->list, (const int*)h->drows, h->pitch, (const int*)h->dRowN, h->mult, h->obs);
	}
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

// host kind: every id inside [0, max_points), and distinct where the call says so
static int cull_check_ids(const mcs_covis* h, const int32_t* ids, int n, bool distinct) {
	for (int i = 0; i < n; ++i)
		if (ids[i] < 0 || ids[i] >= h->maxPts) return fail(MCS_ERR_INVALID, "map point id outside [0, max_points)");
	if (distinct) {
		std::vector<int32_t> v(ids, ids + n);
		std::sort(v.begin(), v.end());
		if (std::adjacent_find(v.begin(), v.end()) != v.end()) return fail(MCS_ERR_INVALID, "a map point is listed twice");
	}
	return MCS_OK;
}

int mcs_covis_observations(mcs_covis* h, const int32_t* ids, int n, mcs_mem_kind kind, int32_t* nobs) {
	if (!h || n < 0 || (n > 0 && (!ids || !nobs))) return fail(MCS_ERR_INVALID, "null argument");
	mcs_ctx* c = h->ctx;
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the observation counts run in order: switch deferred searches off (mcs_ctx_set_async_search)");
	if (n == 0) return MCS_OK;
	if (kind == MCS_MEM_HOST)
		if (int r = cull_check_ids(h, ids, n, false)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	Staging st(c, kind == MCS_MEM_HOST);
	const int* dI = nullptr; int* oN = nullptr;
	st.in(&dI, ids, (size_t)n * 4); st.out(&oN, nobs, (size_t)n * 4);
	if (int r = st.commit()) return r;
	const dim3 g(blocks(n)), b(256);
	hipLaunchKernelGGL(k_cull_pt_mark, g, b, 0, s, dI, n, h->maxPts, h->mult, (unsigned long long*)nullptr);
	cull_observe(h, (int)h->id.size(), s);
	if (h->wide) {
		hipLaunchKernelGGL(k_cull_pt_obs<true>, g, b, 0, s, dI, n, h->maxPts, (const uint8_t*)h->ptBad, (const uint32_t*)h->obs, oN);
		hipLaunchKernelGGL(k_cull_pt_unmark<true>, g, b, 0, s, dI, n, h->maxPts, (const int*)nullptr, h->ptBad, h->mult, (unsigned long long*)nullptr, h->obs);
	} else {
		hipLaunchKernelGGL(k_cull_pt_obs<false>, g, b, 0, s, dI, n, h->maxPts, (const uint8_t*)h->ptBad, (const uint32_t*)h->obs, oN);
		hipLaunchKernelGGL(k_cull_pt_unmark<false>, g, b, 0, s, dI, n, h->maxPts, (const int*)nullptr, h->ptBad, h->mult, (unsigned long long*)nullptr, h->obs);
	}
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_covis_cull_points(mcs_covis* h, int64_t current_kf_id, int n, const int32_t* ids, const int32_t* found, const int32_t* visible, const int64_t* first_kf_id,
                          mcs_mem_kind kind, int32_t* verdict) {
	if (!h || n < 0 || (n > 0 && (!ids || !found || !visible || !first_kf_id || !verdict))) return fail(MCS_ERR_INVALID, "null argument");
	mcs_ctx* c = h->ctx;
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "map points are culled in order: switch deferred searches off (mcs_ctx_set_async_search)");
	if (n == 0) return MCS_OK;
	if (kind == MCS_MEM_HOST)
		if (int r = cull_check_ids(h, ids, n, true)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	Staging st(c, kind == MCS_MEM_HOST);
	const int* dI = nullptr; const int* dF = nullptr; const int* dV = nullptr; const long long* dK = nullptr; int* oV = nullptr;
	st.in(&dI, ids, (size_t)n * 4); st.in(&dF, found, (size_t)n * 4); st.in(&dV, visible, (size_t)n * 4); st.in(&dK, first_kf_id, (size_t)n * 8);
	st.out(&oV, verdict, (size_t)n * 4);
	if (int r = st.commit()) return r;
	const dim3 g(blocks(n)), b(256);
	const unsigned long long cur = (unsigned long long)current_kf_id;
	hipLaunchKernelGGL(k_cull_pt_mark, g, b, 0, s, dI, n, h->maxPts, h->mult, h->key);
	cull_observe(h, (int)h->id.size(), s);
	if (h->wide) {
		hipLaunchKernelGGL(k_cull_pt_verdict<true>, g, b, 0, s, cur, dI, n, dF, dV, dK, h->maxPts, (const uint8_t*)h->ptBad, (const unsigned long long*)h->key, (const uint32_t*)h->obs, oV);
		hipLaunchKernelGGL(k_cull_pt_unmark<true>, g, b, 0, s, dI, n, h->maxPts, (const int*)oV, h->ptBad, h->mult, h->key, h->obs);
	} else {
		hipLaunchKernelGGL(k_cull_pt_verdict<false>, g, b, 0, s, cur, dI, n, dF, dV, dK, h->maxPts, (const uint8_t*)h->ptBad, (const unsigned long long*)h->key, (const uint32_t*)h->obs, oV);
		hipLaunchKernelGGL(k_cull_pt_unmark<false>, g, b, 0, s, dI, n, h->maxPts, (const int*)oV, h->ptBad, h->mult, h->key, h->obs);
	}
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

// ---- cMapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors over the store
int mcs_covis_set_keyframe_descriptors(mcs_covis* h, int64_t mnId, const uint8_t* desc, const uint8_t* mask, int stride, int dim, int n, mcs_mem_kind kind) {
	if (!h || (n > 0 && !desc)) return fail(MCS_ERR_INVALID, "null argument");
	if (dim != 16 && dim != 32 && dim != 64) return fail(MCS_ERR_INVALID, "dim must be 16, 32 or 64");
	if (stride < dim || (stride & 3)) return fail(MCS_ERR_INVALID, "stride must be a multiple of 4 and at least dim");
	const int slot = covis_slot(h, mnId);
	if (slot < 0) return fail(MCS_ERR_INVALID, "keyframe not in the store");
	if (n != h->rowN[slot]) return fail(MCS_ERR_INVALID, "one descriptor row per feature of the keyframe's row");
	if (h->descDim && (h->descDim != dim || h->descMasks != (mask != nullptr)))
		return fail(MCS_ERR_INVALID, "the store's first descriptors fixed another dim, or whether masks exist");
	mcs_ctx* c = h->ctx;
	HIPCHK(hipSetDevice(c->device));
	if (!h->descDim) {
		const size_t bytes = (size_t)h->maxKf * h->pitch * dim;
		if (h->descSlab.reserve(bytes) != hipSuccess || (mask && h->maskSlab.reserve(bytes) != hipSuccess)) {
			(void)hipGetLastError();
			return fail(MCS_ERR_HIP, "descriptor slab allocation failed");
		}
		h->descDim = dim; h->descMasks = mask != nullptr;
	}
	Staging st(c, kind == MCS_MEM_HOST);
	const uint32_t* sD = nullptr; const uint32_t* sM = nullptr;
	st.in(&sD, desc, (size_t)n * stride); st.in(&sM, mask, (size_t)n * stride);
	if (int r = st.commit()) return r;
	if (n > 0) {
		const size_t at = (size_t)slot * h->pitch * dim;
		const unsigned g = blocks((long long)n * (dim / 4));
		hipLaunchKernelGGL(k_mp_set_desc, dim3(g), dim3(256), 0, c->stream, sD, n, stride / 4, dim / 4, (uint32_t*)(h->descSlab.p + at));
		if (mask) hipLaunchKernelGGL(k_mp_set_desc, dim3(g), dim3(256), 0, c->stream, sM, n, stride / 4, dim / 4, (uint32_t*)(h->maskSlab.p + at));
	}
	HIPCHK(hipGetLastError());
	h->hasDesc[slot] = 1;
	return st.finish(MCS_OK);
}

int mcs_covis_update_points(mcs_covis* h, int n, const int32_t* ids, const double* pos, const int64_t* ref_kf, const double* scale_factors, int nlevels,
                            mcs_mem_kind kind, double* normal, double* min_dist, double* max_dist, double* min_inv, double* max_inv, uint8_t* desc, uint8_t* mask,
                            int32_t* n_desc, int64_t* best_kf, int32_t* best_feat, int32_t* status) {
	if (!h || n < 0 || !scale_factors || (n > 0 && (!ids || !pos || !ref_kf))) return fail(MCS_ERR_INVALID, "null argument");
	if (kind == MCS_MEM_HOST && n > 0 && !status) return fail(MCS_ERR_INVALID, "host kind needs the status array");
	if (nlevels < 2 || nlevels > MCS_MAX_LEVELS) return fail(MCS_ERR_INVALID, "nlevels must lie in [2, MCS_MAX_LEVELS]");
	mcs_ctx* c = h->ctx;
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "map points are refreshed in order: switch deferred searches off (mcs_ctx_set_async_search)");
	const int S = (int)h->id.size();
	size_t E = 0;   // the entries of every live row: no segment list can be longer, and nothing is read back to learn the true length
	for (int k = 0; k < S; ++k) {
		if (!h->live[k]) continue;
		E += (size_t)h->rowN[k];
		if (desc && !h->hasDesc[k]) return fail(MCS_ERR_INVALID, "a live keyframe has no stored descriptors (mcs_covis_set_keyframe_descriptors)");
	}
	if (E > 0x7FFFFFFFull) return fail(MCS_ERR_CAPACITY, "the store holds more than 2^31 - 1 observations");
	if (n == 0) return MCS_OK;
	if (kind == MCS_MEM_HOST)
		if (int r = cull_check_ids(h, ids, n, true)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	const bool withDesc = desc != nullptr;   // a store without a live keyframe has no dim yet: every point then collects nothing
	const int dim = h->descDim;
	const bool masks = withDesc && h->descMasks;
	// scratch: the context's grow-only buffer (the calls that share it run in the order of the context's stream)
	Carve cv;
	const size_t N1 = (size_t)n + 1, E1 = std::max<size_t>(E, 1);
	const size_t oSeg = cv.take(N1 * 4), oCur = cv.take(N1 * 4), oOff = cv.take(N1 * 4), oSt = cv.take(N1 * 4), oEnt0 = cv.take(E1 * 8), oEnt1 = cv.take(E1 * 8);
	size_t oCntE = 0, oOffE = 0, oBest = 0, oEntE = 0, oRowsD = 0, oRowsM = 0;
	if (withDesc) {
		oCntE = cv.take(N1 * 4); oOffE = cv.take(N1 * 4); oBest = cv.take(N1 * 4); oEntE = cv.take(E1 * 8); oRowsD = cv.take(E1 * dim);
		if (masks) oRowsM = cv.take(E1 * dim);
	}
	HIPCHK(c->lmBuf.reserve(cv.total));
	uint8_t* b = c->lmBuf.p;
	int* seg = (int*)(b + oSeg); int* cur = (int*)(b + oCur); int* off = (int*)(b + oOff); int* stv = (int*)(b + oSt);
	unsigned long long* ent0 = (unsigned long long*)(b + oEnt0); unsigned long long* ent1 = (unsigned long long*)(b + oEnt1);
	Staging st(c, kind == MCS_MEM_HOST);
	const int* dI = nullptr; const double* dP = nullptr; const long long* dR = nullptr; const double* dSf = nullptr;
	double* oN = nullptr; double* oMn = nullptr; double* oMx = nullptr; double* oMi = nullptr; double* oXi = nullptr; uint8_t* oD = nullptr; uint8_t* oM = nullptr;
	int* oNd = nullptr; long long* oBk = nullptr; int* oBf = nullptr; int* oS = nullptr;
	st.in(&dI, ids, (size_t)n * 4); st.in(&dP, pos, (size_t)n * 24); st.in(&dR, ref_kf, (size_t)n * 8); st.in(&dSf, scale_factors, (size_t)nlevels * 8);
	// an output that is not asked for stays a null pointer in both kinds; the host kind's outputs start from the caller's bytes (entries of status != 0 keep them)
	st.inout(&oN, normal, (size_t)n * 24); st.inout(&oMn, min_dist, (size_t)n * 8); st.inout(&oMx, max_dist, (size_t)n * 8); st.inout(&oMi, min_inv, (size_t)n * 8);
	st.inout(&oXi, max_inv, (size_t)n * 8); st.inout(&oNd, n_desc, (size_t)n * 4); st.inout(&oBk, best_kf, (size_t)n * 8); st.inout(&oBf, best_feat, (size_t)n * 4);
	st.inout(&oS, status, (size_t)n * 4);
	if (withDesc) { st.inout(&oD, desc, (size_t)n * dim); if (masks) st.inout(&oM, mask, (size_t)n * dim); }
	if (int r = st.commit()) return r;
	const dim3 gn(blocks(n)), gw(blocks((long long)n * 64)), gs(blocks((long long)std::max(S, 1) * 64)), tb(256);
	HIPCHK(hipMemsetAsync(seg, 0, N1 * 4, s));
	HIPCHK(hipMemsetAsync(cur, 0, N1 * 4, s));
	hipLaunchKernelGGL(k_mp_mark, gn, tb, 0, s, dI, n, h->maxPts, h->mult);
	c->tic("mp_count");
	if (S > 0) hipLaunchKernelGGL(k_mp_stream<false>, gs, tb, 0, s, (const int*)h->rows, h->pitch, (const int*)h->dRowN, (const uint8_t*)h->dLive, (const int*)h->mult, S, seg, (const int*)off, ent0);
	c->toc("mp_count");
	hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(1024), 0, s, (const int*)seg, n, off, off + n);
	c->tic("mp_fill");
	if (S > 0) hipLaunchKernelGGL(k_mp_stream<true>, gs, tb, 0, s, (const int*)h->rows, h->pitch, (const int*)h->dRowN, (const uint8_t*)h->dLive, (const int*)h->mult, S, cur, (const int*)off, ent0);
	c->toc("mp_fill");
	c->tic("mp_sort");
	hipLaunchKernelGGL(k_mp_sort, dim3(n), tb, 0, s, (const int*)off, (const unsigned long long*)ent0, ent1);
	c->toc("mp_sort");
	c->tic("mp_normal");
	hipLaunchKernelGGL(k_mp_normal, gw, tb, 0, s, dI, n, h->maxPts, (const uint8_t*)h->ptBad, (const int*)h->mult, (const int*)off, (const unsigned long long*)ent1, dP, dR,
	                   (const long long*)h->dIds, (const uint8_t*)h->dLive, S, (const double*)h->dT, (const uint8_t*)h->octs, h->pitch, dSf, nlevels, stv, oN, oMn, oMx, oMi, oXi, oS);
	c->toc("mp_normal");
	if (withDesc) {
		int* cntE = (int*)(b + oCntE); int* offE = (int*)(b + oOffE); int* best = (int*)(b + oBest); unsigned long long* entE = (unsigned long long*)(b + oEntE);
		uint8_t* rowsD = b + oRowsD; uint8_t* rowsM = masks ? b + oRowsM : nullptr;
		const uint8_t* slabM = masks ? h->maskSlab.p : nullptr;
		c->tic("mp_collect");
		hipLaunchKernelGGL(k_mp_collect, gw, tb, 0, s, dI, n, h->maxPts, (const uint8_t*)h->ptBad, (const int*)h->mult, (const int*)off, (const unsigned long long*)ent1,
		                   (const uint8_t*)h->dKfBad, h->pitch, dim, (const uint8_t*)h->descSlab.p, slabM, cntE, (const int*)offE, entE, rowsD, rowsM, 0);
		hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(1024), 0, s, (const int*)cntE, n, offE, offE + n);
		hipLaunchKernelGGL(k_mp_collect, gw, tb, 0, s, dI, n, h->maxPts, (const uint8_t*)h->ptBad, (const int*)h->mult, (const int*)off, (const unsigned long long*)ent1,
		                   (const uint8_t*)h->dKfBad, h->pitch, dim, (const uint8_t*)h->descSlab.p, slabM, cntE, (const int*)offE, entE, rowsD, rowsM, 1);
		c->toc("mp_collect");
		DistinctArgs a{};
		a.desc = rowsD; a.mask = rowsM; a.stride = dim; a.dim = dim; a.offsets = offE; a.npoints = n; a.bestIdx = best;
		c->tic("mp_distinct");
		launch_distinct(a, s);
		c->toc("mp_distinct");
		hipLaunchKernelGGL(k_mp_winner, gn, tb, 0, s, dI, n, (const int*)stv, (const int*)h->mult, (const int*)offE, (const unsigned long long*)entE, (const int*)best,
		                   (const long long*)h->dIds, dim, (const uint8_t*)rowsD, (const uint8_t*)rowsM, (uint32_t*)oD, (uint32_t*)oM, oNd, oBk, oBf);
	}
	hipLaunchKernelGGL(k_covis_unmark, gn, tb, 0, s, dI, n, h->maxPts, h->mult);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}
