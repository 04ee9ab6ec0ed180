// mcs_mappoints.hip — refreshing map points from the covisibility store (mcs_covis.h):
//   cMapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors for a list of points    src/cMapPoint.cpp:449-492, 294-388 (mcs_covis_update_points)
// mult[p] = 1 + the LAST list index that names p (atomicMax: any order gives the same): that entry owns the point's segment, every copy reads it.
// A segment = the (slot << 32 | feature) entries of every live row that name the point, sorted: ascending slot, ascending feature within a slot.
#include "mcs_covis.h"

namespace mcs {
namespace {

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
__global__ __launch_bounds__(256) void k_mp_stream(CovisView s, const int* __restrict__ mult, int* seg, const int* __restrict__ off, unsigned long long* ent) {
	const int slot = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (slot >= s.nslots || !s.live[slot]) return;
	walk_row<false>(s.row(slot), nullptr, s.rowN[slot], lane, [&](int p, int j, int q, unsigned) {
		const int m = mult[p];
		if (!m) return;
		if (FILL) ent[off[m - 1] + atomicAdd(&seg[m - 1], 1)] = ((unsigned long long)slot << 32) | (unsigned)(4 * j + q);
		else atomicAdd(&seg[m - 1], 1);
	});
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
// k_mp_normal and k_mp_collect take the store's arrays as `const __restrict__` arguments of their own, not as a CovisView: they read four or five of its
// fields, and with the view the serial chain below waited for all six shuffles before its first addition (a kernel argument load left pending on one path into the
// loop) and k_mp_collect fetched four lines of arguments per wave for two: 3 - 4 % and 2 - 3 % slower on an MI355X (profiles/NOTES.md).
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

}  // namespace
}  // namespace mcs

using namespace mcs;

int mcs_covis_set_keyframe_descriptors(mcs_covis* h, int64_t mnId, const uint8_t* desc, const uint8_t* mask, int stride, int dim, int n, mcs_mem_kind kind) {
	if (!h || (n > 0 && !desc)) return fail(MCS_ERR_INVALID, "null argument");
	if (dim != 16 && dim != 32 && dim != 64) return fail(MCS_ERR_INVALID, "dim must be 16, 32 or 64");
	if (stride < dim || (stride & 3)) return fail(MCS_ERR_INVALID, "stride must be a multiple of 4 and at least dim");
	int slot;
	if (int r = covis_slots_of(h, &mnId, 1, &slot)) return r;
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
		const size_t at = h->at(slot) * dim;
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
	const int S = h->slots();
	size_t E = 0;   // the entries of every live row: no segment list can be longer, and nothing is read back to learn the true length
	for (int k = 0; k < S; ++k) {
		if (!h->live[k]) continue;
		E += (size_t)h->rowN[k];
		if (desc && !h->hasDesc[k]) return fail(MCS_ERR_INVALID, "a live keyframe has no stored descriptors (mcs_covis_set_keyframe_descriptors)");
	}
	if (E > 0x7FFFFFFFull) return fail(MCS_ERR_CAPACITY, "the store holds more than 2^31 - 1 observations");
	if (n == 0) return MCS_OK;
	if (kind == MCS_MEM_HOST)
		if (int r = check_point_ids(h, ids, n, 0, true)) return r;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	const bool withDesc = desc != nullptr;   // a store without a live keyframe has no dim yet: every point then collects nothing
	const int dim = h->descDim;
	const bool masks = withDesc && h->descMasks;
	// scratch: the context's grow-only buffer (the calls that share it run in the order of the context's stream)
	const size_t N1 = (size_t)n + 1, E1 = std::max<size_t>(E, 1);
	int* seg = nullptr; int* cur = nullptr; int* off = nullptr; int* stv = nullptr; unsigned long long* ent0 = nullptr; unsigned long long* ent1 = nullptr;
	int* cntE = nullptr; int* offE = nullptr; int* best = nullptr; unsigned long long* entE = nullptr; uint8_t* rowsD = nullptr; uint8_t* rowsM = nullptr;
	Layout lay;
	lay.piece(&seg, N1 * 4); lay.piece(&cur, N1 * 4); lay.piece(&off, N1 * 4); lay.piece(&stv, N1 * 4); lay.piece(&ent0, E1 * 8); lay.piece(&ent1, E1 * 8);
	if (withDesc) {
		lay.piece(&cntE, N1 * 4); lay.piece(&offE, N1 * 4); lay.piece(&best, N1 * 4); lay.piece(&entE, E1 * 8); lay.piece(&rowsD, E1 * dim);
		if (masks) lay.piece(&rowsM, E1 * dim);
	}
	HIPCHK(c->lmBuf.reserve(lay.total));
	lay.place(c->lmBuf.p);
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
	const CovisView v = h->view(S);
	const dim3 gn(blocks(n)), gw(blocks((long long)n * 64)), gs(blocks((long long)std::max(S, 1) * 64)), tb(256);
	HIPCHK(hipMemsetAsync(seg, 0, N1 * 4, s));
	HIPCHK(hipMemsetAsync(cur, 0, N1 * 4, s));
	hipLaunchKernelGGL(k_mp_mark, gn, tb, 0, s, dI, n, h->maxPts, h->mult);
	c->tic("mp_count");
	if (S > 0) hipLaunchKernelGGL(k_mp_stream<false>, gs, tb, 0, s, v, h->mult, seg, off, ent0);
	c->toc("mp_count");
	hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(1024), 0, s, seg, n, off, off + n);
	c->tic("mp_fill");
	if (S > 0) hipLaunchKernelGGL(k_mp_stream<true>, gs, tb, 0, s, v, h->mult, cur, off, ent0);
	c->toc("mp_fill");
	c->tic("mp_sort");
	hipLaunchKernelGGL(k_mp_sort, dim3(n), tb, 0, s, off, ent0, ent1);
	c->toc("mp_sort");
	c->tic("mp_normal");
	hipLaunchKernelGGL(k_mp_normal, gw, tb, 0, s, dI, n, h->maxPts, h->ptBad, h->mult, off, ent1, dP, dR, h->dIds, h->dLive, S, h->dT, h->octs, h->pitch, dSf, nlevels, stv,
	                   oN, oMn, oMx, oMi, oXi, oS);
	c->toc("mp_normal");
	if (withDesc) {
		const uint8_t* slabM = masks ? h->maskSlab.p : nullptr;
		c->tic("mp_collect");
		hipLaunchKernelGGL(k_mp_collect, gw, tb, 0, s, dI, n, h->maxPts, h->ptBad, h->mult, off, ent1, h->dKfBad, h->pitch, dim, h->descSlab.p, slabM, cntE, offE, entE, rowsD,
		                   rowsM, 0);
		hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(1024), 0, s, cntE, n, offE, offE + n);
		hipLaunchKernelGGL(k_mp_collect, gw, tb, 0, s, dI, n, h->maxPts, h->ptBad, h->mult, off, ent1, h->dKfBad, h->pitch, dim, h->descSlab.p, slabM, cntE, offE, entE, rowsD,
		                   rowsM, 1);
		c->toc("mp_collect");
		DistinctArgs a{};
		a.desc = rowsD; a.mask = rowsM; a.stride = dim; a.dim = dim; a.offsets = offE; a.npoints = n; a.bestIdx = best;
		c->tic("mp_distinct");
		launch_distinct(a, s);
		c->toc("mp_distinct");
		hipLaunchKernelGGL(k_mp_winner, gn, tb, 0, s, dI, n, stv, h->mult, offE, entE, best, h->dIds, dim, rowsD, rowsM, (uint32_t*)oD, (uint32_t*)oM, oNd, oBk, oBf);
	}
	hipLaunchKernelGGL(k_covis_unmark, gn, tb, 0, s, dI, n, h->maxPts, h->mult);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}
