// mcs_cull.hip — keyframe and map point culling on the covisibility store (mcs_covis.h):
//   cLocalMapping::KeyFrameCulling / MapPointCulling                src/cLocalMapping.cpp:517-593, 187-221 (mcs_covis_cull_keyframes / _cull_points)
//   cMapPoint::Observations                                         src/cMapPoint.cpp:158-162              (mcs_covis_observations)
// obs[p][level] = the live keyframes whose FIRST entry of point p (the distinct row's) lies at that octave: MCS_MAX_LEVELS counters per point, 16 bits each
// packed two to a word while the store has fewer than 65 536 slots (WIDE = false), 32 bits otherwise.  Observations() is the sum of a point's counters.  The
// table is zero between calls: a call marks the points it asks about (mult), counts those, and clears exactly those again.
#include "mcs_covis.h"

namespace mcs {
namespace {

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
__global__ __launch_bounds__(256) void k_cull_mark_rows(CovisView s, const int* list, int* mult) {
	const int slot = list[blockIdx.x] & kListSlot, f = blockIdx.y * 256 + threadIdx.x;
	if (f >= s.rowN[slot]) return;
	const int p = s.drow(slot)[f];
	if (p >= 0) mult[p] = 1;
}
template <bool WIDE>
__global__ __launch_bounds__(256) void k_cull_unmark_rows(CovisView s, const int* list, int* mult, uint32_t* obs) {
	const int slot = list[blockIdx.x] & kListSlot, f = blockIdx.y * 256 + threadIdx.x;
	if (f >= s.rowN[slot]) return;
	const int p = s.drow(slot)[f];
	if (p >= 0) { mult[p] = 0; obs_zero<WIDE>(obs, p); }
}
// The wide pass: one wave per slot, the walk of k_covis_count with the octave row alongside (one 4-byte load per 16-byte load of ids); every entry that names
// a marked point adds one to that point's counter of the entry's level.  Bad keyframes observe (the reference has no test there), erased slots do not.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_cull_observe(CovisView s, const int* __restrict__ mult, uint32_t* __restrict__ obs) {
	const int slot = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (slot >= s.nslots || !s.live[slot]) return;
	walk_row<true>(s.drow(slot), s.oct(slot), s.rowN[slot], lane, [&](int p, int, int, unsigned level) { if (mult[p]) obs_atomic_inc<WIDE>(obs, p, level); });
}
// The serial chain (src/cLocalMapping.cpp:527-591): ONE workgroup judges the listed keyframes one after another, because a culled keyframe changes what the
// next one sees.  Per keyframe: (1) take its own observations out of the table (:561-562, pKF never counts; the distinct row holds each point once, at its
// first level); (2) per feature of the full row: nMPs, Observations() - 1 >= 3, nObs = the counters up to octave + 1 >= 5 (:538-587); (3) decide (:589);
// (4) culled: the observations stay out, every point left with two or fewer observers goes bad and is emitted in feature order
// (src/cMultiKeyFrame.cpp:591-593, src/cMapPoint.cpp:96-116, 185-204) — otherwise put the observations back.  The table, ptBad and the outputs are touched by
// this workgroup alone; a barrier with a workgroup fence separates the phases.  A point that went bad is skipped by every later keyframe through ptBad, which
// is what nulling its entries does in the reference.
template <bool WIDE>
__global__ __launch_bounds__(1024) void k_cull_chain(CovisView s, const int* __restrict__ list, int n, uint8_t* ptBad, uint8_t* kfBad, uint32_t* obs, int cap,
                                                      int* verdict, int* nMps, int* nRed, int* badPoints, int* nBad) {
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
		const int nrow = s.len(slot);
		const int* row = s.row(slot);
		const int* drow = s.drow(slot);
		const uint8_t* oct = s.oct(slot);
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
				const int rank = block_rank(goes, wE, base);
				if (goes) {
					ptBad[p] = 1;
					if (rank < cap) badPoints[rank] = p;
				}
				block_carry(wE, base);
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
__global__ __launch_bounds__(256) void k_cull_pt_obs(CovisView s, const int* ids, int n, const uint32_t* obs, int* nobs) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = ids[i];
	int all = 0, pre = 0;
	if ((unsigned)p < (unsigned)s.maxPoints && !s.ptBad[p]) obs_sums<WIDE>(obs, p, 0, all, pre);   // a bad point has no observations (src/cMapPoint.cpp:193)
	nobs[i] = all;
}
template <bool WIDE>
__global__ __launch_bounds__(256) void k_cull_pt_verdict(CovisView s, unsigned long long cur, const int* ids, int n, const int* found, const int* visible,
                                                          const long long* firstKf, const unsigned long long* key, const uint32_t* obs, int* verdict) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int p = ids[i];
	int r = 1;
	if ((unsigned)p < (unsigned)s.maxPoints && !s.ptBad[p]) {   // :195
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

}  // namespace
}  // namespace mcs

using namespace mcs;

int mcs_covis_set_keyframe_octaves(mcs_covis* h, int64_t mnId, const uint8_t* octaves, int n, mcs_mem_kind kind) {
	if (!h || (n > 0 && !octaves)) return fail(MCS_ERR_INVALID, "null argument");
	int slot;
	if (int r = covis_slots_of(h, &mnId, 1, &slot)) return r;
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
	hipLaunchKernelGGL(k_cull_set_octaves, dim3(blocks(h->pitch)), dim3(256), 0, c->stream, src, n, h->pitch, h->octs + h->at(slot));
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

// the wide pass over every slot; the marked points' counters are complete behind it
static void cull_observe(mcs_covis* h, int S, hipStream_t s) {
	if (S <= 0) return;
	h->ctx->tic("cull_observe");
	LAUNCH_BY_WIDTH(h, k_cull_observe, dim3(blocks((long long)S * 64)), dim3(256), s, h->view(S), h->mult, h->obs);
	h->ctx->toc("cull_observe");
}

int mcs_covis_cull_keyframes(mcs_covis* h, int n, const int64_t* mnIds, const uint8_t* not_erase, int cap, mcs_mem_kind kind, int32_t* verdict, int32_t* n_mps,
                             int32_t* n_redundant, int32_t* bad_points, int32_t* n_bad_points) {
	if (!h || !n_bad_points || n < 0 || cap < 0 || (n > 0 && (!mnIds || !verdict || !n_mps || !n_redundant)) || (cap > 0 && !bad_points))
		return fail(MCS_ERR_INVALID, "null argument / bad sizes");
	mcs_ctx* c = h->ctx;
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "keyframes are culled in order: switch deferred searches off (mcs_ctx_set_async_search)");
	const int S = h->slots();
	std::vector<int> list(n);
	std::vector<uint8_t> seen(S, 0);
	int maxRow = 0;
	for (int k = 0; k < n; ++k) {   // keyframe by keyframe: the first offending entry decides which refusal the caller reads
		int slot;
		if (int r = covis_slots_of(h, mnIds + k, 1, &slot)) return r;
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
	const CovisView v = h->view(S);
	const dim3 gl((unsigned)std::max(n, 1), blocks(std::max(maxRow, 1)));
	const bool rowsToMark = n > 0 && maxRow > 0;
	if (rowsToMark) {
		hipLaunchKernelGGL(k_cull_mark_rows, gl, dim3(256), 0, s, v, h->list, h->mult);
		cull_observe(h, S, s);
	}
	c->tic("cull_chain");
	LAUNCH_BY_WIDTH(h, k_cull_chain, dim3(1), dim3(1024), s, v, h->list, n, h->ptBad, h->dKfBad, h->obs, cap, oV, oM, oR, oB, oNb);
	c->toc("cull_chain");
	if (rowsToMark) LAUNCH_BY_WIDTH(h, k_cull_unmark_rows, gl, dim3(256), s, v, h->list, h->mult, h->obs);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_covis_observations(mcs_covis* h, const int32_t* ids, int n, mcs_mem_kind kind, int32_t* nobs) {
	if (!h || n < 0 || (n > 0 && (!ids || !nobs))) return fail(MCS_ERR_INVALID, "null argument");
	mcs_ctx* c = h->ctx;
	if (c->asyncSearch) return fail(MCS_ERR_UNSUPPORTED, "the observation counts run in order: switch deferred searches off (mcs_ctx_set_async_search)");
	if (n == 0) return MCS_OK;
	if (kind == MCS_MEM_HOST)
		if (int r = check_point_ids(h, ids, n, 0, false)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	Staging st(c, kind == MCS_MEM_HOST);
	const int* dI = nullptr; int* oN = nullptr;
	st.in(&dI, ids, (size_t)n * 4); st.out(&oN, nobs, (size_t)n * 4);
	if (int r = st.commit()) return r;
	const dim3 g(blocks(n)), b(256);
	hipLaunchKernelGGL(k_cull_pt_mark, g, b, 0, s, dI, n, h->maxPts, h->mult, nullptr);   // no key: the points are not ranked
	cull_observe(h, h->slots(), s);
	LAUNCH_BY_WIDTH(h, k_cull_pt_obs, g, b, s, h->view(h->slots()), dI, n, h->obs, oN);
	LAUNCH_BY_WIDTH(h, k_cull_pt_unmark, g, b, s, dI, n, h->maxPts, nullptr, h->ptBad, h->mult, nullptr, h->obs);   // no verdict, no key
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
		if (int r = check_point_ids(h, ids, n, 0, true)) return r;
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
	cull_observe(h, h->slots(), s);
	LAUNCH_BY_WIDTH(h, k_cull_pt_verdict, g, b, s, h->view(h->slots()), cur, dI, n, dF, dV, dK, h->key, h->obs, oV);
	LAUNCH_BY_WIDTH(h, k_cull_pt_unmark, g, b, s, dI, n, h->maxPts, oV, h->ptBad, h->mult, h->key, h->obs);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}
