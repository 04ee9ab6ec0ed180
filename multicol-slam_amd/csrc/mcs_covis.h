// mcs_covis.h — the device store behind mcs_covis_* and what its stages share (DESIGN.md sections 4h-4j).  Included by mcs_covis.hip (the store, the local map
// and the covisibility counts), mcs_cull.hip (keyframe and map point culling) and mcs_mappoints.hip (refreshing map points) only.
//
// THE SCRATCH INVARIANT.  Three per-point tables of the store are scratch that every stage borrows: between calls
//     mult[p] == 0,   key[p] == ~0 (kNoKey),   every counter of obs[p] == 0        for every point p.
// A call marks the points it asks about, works on those, and puts exactly those back before it returns (the unmark / reset kernel at the end of its chain
// walks the same list or the same rows as the mark kernel at its start).  Every runtime call that can fail (allocation, Staging::commit, a memset) is placed
// BEFORE the first mark, so a call that fails leaves no marks behind; behind the first mark there are only kernel launches.  A stage that breaks this
// breaks the NEXT call of another stage, not its own: tests/test_gpu_covis_rotation.py runs the stages in rotation on one store for that reason.
#pragma once
#include "mcs_host.h"
#include <unordered_map>

namespace mcs {

constexpr unsigned long long kNoKey = ~0ull;

// What the kernels read of a store, passed BY VALUE.  Rows, distinct rows and octave rows share one slot layout (`pitch` entries per slot, a multiple of 4, so
// every row starts 16-byte aligned); row() / drow() / oct() are the only place that knows it.  Kernels that write ptBad / kfBad take those as arguments of
// their own.
struct CovisView {
	const int* rows; const int* drows; const uint8_t* octs;
	const int* rowN; const uint8_t* live; const uint8_t* kfBad; const long long* ids; const double* t;   // per slot; t = 3 doubles
	const uint8_t* ptBad;                                                                                  // per point
	int pitch, nslots, maxPoints;
	__host__ __device__ size_t at(int slot) const { return (size_t)slot * pitch; }
	__host__ __device__ const int* row(int slot) const { return rows + at(slot); }
	__host__ __device__ const int* drow(int slot) const { return drows + at(slot); }
	__host__ __device__ const uint8_t* oct(int slot) const { return octs + at(slot); }
	// rowN[slot] for a kernel that also stores and has barriers (k_cull_chain): no kernel that takes a view writes rowN, which a pointer inside a by-value struct
	// cannot say (`const __restrict__` only counts on a kernel argument); read through the constant address space the wave-uniform load stays a scalar load
	__device__ int len(int slot) const { return *(const __attribute__((address_space(4))) int*)(rowN + slot); }
};

__device__ __forceinline__ int wave_sum(int v) {
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	return v;
}
__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }
inline unsigned blocks(long long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// The one-wave-per-slot walk: lane `lane` of the wave streams the row 16 bytes per load (quads lane, lane + 64, ... of the (n + 3) / 4 the row holds; the
// padding up to the pitch reads -1) and calls f(p, j, q, level) for every component q of quad j that names a point: feature 4 * j + q.  OCT: the row's octaves
// are read alongside, ONE 4-byte word per 16-byte load, and level = its byte q; without OCT `oct` is not read and level is 0.
template <bool OCT, class F>
__device__ __forceinline__ void walk_row(const int* row, const uint8_t* oct, int n, int lane, F f) {
	const int n4 = (n + 3) >> 2;
	const int4* r = reinterpret_cast<const int4*>(row);
	const uint32_t* o = reinterpret_cast<const uint32_t*>(oct);
	for (int j = lane; j < n4; j += 64) {
		const int4 v = r[j];
		const uint32_t l = OCT ? o[j] : 0u;
		if (v.x >= 0) f(v.x, j, 0, l & 0xFFu);
		if (v.y >= 0) f(v.y, j, 1, (l >> 8) & 0xFFu);
		if (v.z >= 0) f(v.z, j, 2, (l >> 16) & 0xFFu);
		if (v.w >= 0) f(v.w, j, 3, l >> 24);
	}
}

// The ranking of a workgroup of 1024 threads that walks a list 1024 entries at a time (wtot: 16 ints of LDS, base: one, zero at the start and published by a
// barrier).  block_rank: the number of takers before this thread, earlier rounds included; ONE barrier.  block_carry: adds the round's takers to `base`; TWO
// barriers, what is written between the two calls needs none of its own.  Every thread of the workgroup calls both, in every round.
__device__ __forceinline__ int block_before(const int* wtot, int base) {   // what the earlier rounds and the waves before this one hold
	for (int j = 0; j < (int)(threadIdx.x >> 6); ++j) base += wtot[j];
	return base;
}
__device__ __forceinline__ int block_rank(bool take, int* wtot, const int& base) {
	const unsigned long long b = __ballot(take);
	if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = __popcll(b);
	__syncthreads();
	return block_before(wtot, base) + __popcll(b & lanes_below());
}
__device__ __forceinline__ void block_carry(const int* wtot, int& base) {
	__syncthreads();
	if (threadIdx.x == 0) { int t = 0; for (int j = 0; j < 16; ++j) t += wtot[j]; base += t; }
	__syncthreads();
}

// used by more than one stage, defined in mcs_covis.hip
__global__ void k_covis_unmark(const int* voter, int n, int maxPoints, int* mult);   // mult[p] = 0 for the listed points
__global__ void k_covis_scan(const int* cnt, int nslots, int* off, int* total);      // exclusive scan in one workgroup; *total = the sum

}  // namespace mcs

// a `template <bool WIDE>` kernel by the store's counter width
#define LAUNCH_BY_WIDTH(h, kernel, grid, block, stream, ...)                                             \
	do {                                                                                                   \
		if ((h)->wide) hipLaunchKernelGGL(kernel<true>, grid, block, 0, stream, __VA_ARGS__);              \
		else hipLaunchKernelGGL(kernel<false>, grid, block, 0, stream, __VA_ARGS__);                       \
	} while (0)

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

	int slots() const { return (int)id.size(); }
	mcs::CovisView view(int nslots) const { return mcs::CovisView{rows, drows, octs, dRowN, dLive, dKfBad, dIds, dT, ptBad, pitch, nslots, maxPts}; }
	size_t at(int slot) const { return view(0).at(slot); }   // where the host writes a slot's rows (and, times dim, its descriptor rows)
};

// the slot of a live keyframe, or -1
inline int covis_slot(const mcs_covis* h, int64_t id) {
	auto it = h->slotOf.find(id);
	return (it == h->slotOf.end() || !h->live[it->second]) ? -1 : it->second;
}
// out[i] = the slot of keyframe ids[i]; refuses an id that is not a live keyframe of the store
int covis_slots_of(const mcs_covis* h, const int64_t* ids, int n, int* out);
// host-kind ids: every one inside [lowest, max_points) (lowest = -1 admits NULL entries), and distinct where the call says so
int check_point_ids(const mcs_covis* h, const int32_t* ids, int n, int lowest, bool distinct);
