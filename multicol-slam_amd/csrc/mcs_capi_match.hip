// mcs_capi_match.hip — matcher half of the C ABI: top-K Hamming lists, the three brute-force searches of cORBmatcher and the single-purpose descriptor calls
// (distances, valid rows, the distinctive descriptor of a map point, the reciprocal self-test).
#include "mcs_host.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace mcs {
void launch_single_distance(const uint8_t* a, const uint8_t* b, const uint8_t* ma, const uint8_t* mb, int dim, int* out, hipStream_t s);
void launch_rows_valid(const int* nkp, int nimg, int cap, uint8_t* valid, hipStream_t s);
void launch_rig_pack_headers(const int* nkp, int nimg, int cap, uint8_t* blocks, int rowStride, hipStream_t s);
void launch_rig_rows_valid(const uint8_t* blocks, int nimg, int cap, int rowStride, uint8_t* valid, int* nkpOut, hipStream_t s);
void launch_selftest_recip(unsigned long long seed, int n, int* mismatches, hipStream_t s);
}
using namespace mcs;

struct DevSets {   // device views of a (query sets, train sets) pair
	const uint8_t *qd, *qm, *qvalid; const int* qgroup;
	const uint8_t *td, *tm, *tvalid; const int* tgroup;
	size_t qInter, tInter;   // host kind, descriptor | mask interleaved in one row: the mask's offset in the staged row
	void resolve() { if (qInter) qm = qd + qInter; if (tInter) tm = td + tInter; }   // after Staging::commit
};

// How the nsets (query set, train set) pairs of one call map onto the caller's arrays: pair s reads query set (s % qmod) and train set (s / tdiv);
// nq_sets / nt_sets = number of distinct sets behind each pointer (what a host-kind call has to stage).
struct SetGrid { int nsets, qmod, tdiv, nq_sets, nt_sets; int toff = 0, tmod = 0x7FFFFFFF; };
static size_t set_span(const mcs_desc_set* d) {   // rows from a set's first to one past its last row
	if (d->block_rows == 0 || d->n == 0) return (size_t)d->n;
	return (size_t)(d->n / d->block_rows - 1) * (size_t)d->block_pitch_rows + (size_t)d->block_rows;
}
static SetGrid grid_batched(int nsets, size_t qpitch, size_t tpitch) { SetGrid g; g.nsets = nsets; g.qmod = nsets; g.tdiv = 1; g.nq_sets = qpitch ? nsets : 1; g.nt_sets = tpitch ? nsets : 1; return g; }
static SetGrid grid_sweep(int nq_sets, int nt_sets) { SetGrid g; g.nsets = nq_sets * nt_sets; g.qmod = nq_sets; g.tdiv = nq_sets; g.nq_sets = nq_sets; g.nt_sets = nt_sets; return g; }
// pairs (frame first + s, its predecessor in a ring of `total` frames), s = 0 .. count-1; both pointers at frame 0 of the ring
static SetGrid grid_ring(int total, int first, int count) { SetGrid g; g.nsets = count; g.qmod = count; g.tdiv = 1; g.nq_sets = total; g.nt_sets = total; g.toff = first + total - 1; g.tmod = total; return g; }

static int validate_sets(mcs_ctx* c, int nsets, const mcs_desc_set* q, const mcs_desc_set* t, int dim, int K) {
	if (!c || !q || !t) return fail(MCS_ERR_INVALID, "null argument");
	if (dim != 16 && dim != 32 && dim != 64) return fail(MCS_ERR_INVALID, "dim must be 16, 32 or 64");
	if (K != 1 && K != 2 && K != 4 && K != 8 && K != 16 && K != 32) return fail(MCS_ERR_INVALID, "K must be 1,2,4,8,16 or 32");
	if (nsets < 1 || q->n < 0 || t->n < 0 || t->n >= (1 << 20)) return fail(MCS_ERR_INVALID, "bad set size (train rows must be < 2^20)");
	if (q->stride < dim || t->stride < dim || (q->stride & 3) || (t->stride & 3)) return fail(MCS_ERR_INVALID, "descriptor stride must be >= dim and a multiple of 4");
	if ((q->mask == nullptr) != (t->mask == nullptr)) return fail(MCS_ERR_INVALID, "masks must be given for both sets or neither");
	if ((q->n > 0 && !q->desc) || (t->n > 0 && !t->desc)) return fail(MCS_ERR_INVALID, "null descriptors");
	for (const mcs_desc_set* d : {q, t})
		if (d->block_rows != 0 && (d->block_rows < 1 || d->n % d->block_rows != 0 || d->block_pitch_rows < d->block_rows))
			return fail(MCS_ERR_INVALID, "block_rows must divide n and block_pitch_rows must be >= block_rows");
	return MCS_OK;
}

namespace mcs {
__global__ __launch_bounds__(256) void k_search_out(int* __restrict__ dm, const int* __restrict__ sm, size_t n, int* __restrict__ dn, const int* __restrict__ sn, int* __restrict__ df,
                                                    const int* __restrict__ sf, int nsets) {
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dm[i] = sm[i];
	if (blockIdx.x == 0)
		for (int i = threadIdx.x; i < nsets; i += 256) { dn[i] = sn[i]; if (df) df[i] = sf[i]; }
}
}  // namespace mcs
static void launch_search_out(int* dm, const int* sm, size_t n, int* dn, const int* sn, int* df, const int* sf, int nsets, hipStream_t s) {
	const int blocks = (int)std::min<size_t>(std::max<size_t>((n + 1023) / 1024, 1), 64);
	hipLaunchKernelGGL(mcs::k_search_out, dim3(blocks), dim3(256), 0, s, dm, sm, n, dn, sn, df, sf, nsets);
}

// host kind: the sets' arrays (and the rays / essential matrices of the triangulation search) declared on the call's staging; device pointers pass through
static int stage_sets(Staging& st, const SetGrid& sg, const mcs_desc_set* q, size_t qpitch, const mcs_desc_set* t, size_t tpitch, DevSets* out,
                      const double** rays1, const double** rays2, const double** E, size_t nE) {
	const size_t qRows = qpitch * (sg.nq_sets - 1) + set_span(q), tRows = tpitch * (sg.nt_sets - 1) + set_span(t);
	// descriptor | mask interleaved in one row (the rig's exchange blocks): the mask rides along with the descriptor copy
	const bool qInter = st.host && q->mask && q->mask > q->desc && q->mask - q->desc < q->stride, tInter = st.host && t->mask && t->mask > t->desc && t->mask - t->desc < t->stride;
	st.in(&out->qd, q->desc, qRows * q->stride);
	if (qInter) out->qInter = q->mask - q->desc; else st.in(&out->qm, q->mask, qRows * q->stride);
	st.in(&out->qvalid, q->valid, qRows); st.in(&out->qgroup, q->group, qRows * 4);
	st.in(&out->td, t->desc, tRows * t->stride);
	if (tInter) out->tInter = t->mask - t->desc; else st.in(&out->tm, t->mask, tRows * t->stride);
	st.in(&out->tvalid, t->valid, tRows); st.in(&out->tgroup, t->group, tRows * 4);
	if (rays1) st.in(rays1, *rays1, qRows * 24);
	if (rays2) st.in(rays2, *rays2, tRows * 24);
	if (E) st.in(E, *E, nE * 8);
	if (st.host) HIPCHK(hipStreamSynchronize(st.c->stream));   // device-kind work enqueued earlier completes before the block may regrow (part of the measured latency path)
	return MCS_OK;
}

static int run_topk(mcs_ctx* c, const DevSets& d, const SetGrid& sg, const mcs_desc_set* q, size_t qpitch, const mcs_desc_set* t, size_t tpitch, int dim,
                    int K, int count_thresh, int max_dist, int* outDist, int* outIdx, int* outCount, hipStream_t ls = nullptr, int slot = 0) {
	MatchArgs a{};
	const int nsets = sg.nsets;
	a.maxDist = max_dist;
	// deferred (ls = the greedy stream): the lists run there, ordered behind the previous search by the stream itself and behind the caller's stream by
	// an event recorded AFTER the train sets' pass, which stays on the caller's stream — 30 us there, and the matcher starts together with whatever the
	// caller enqueues next (started 40 us later it found the chip full of the next batch's FAST workgroups: 0.72 instead of 0.30 ms)
	const bool deferred = ls != nullptr;
	if (!deferred) ls = c->stream;
	if (!deferred) if (int r = ctx_join_greedy(c, c->stream)) return r;   // the previous search's greedy pass still reads the list buffer
	DevBuf& keys = slot ? c->topKeys2 : c->topKeys;
	HIPCHK(keys.reserve(std::max<size_t>((size_t)nsets * q->n, 1) * K * sizeof(uint32_t)));
	a.keys = keys.as<uint32_t>();
	a.qd = d.qd; a.qm = d.qm; a.qvalid = d.qvalid; a.qgroup = d.qgroup; a.td = d.td; a.tm = d.tm; a.tvalid = d.tvalid; a.tgroup = d.tgroup;
	a.nq = q->n; a.nt = t->n; a.qstride = q->stride; a.tstride = t->stride; a.qpitch = qpitch; a.tpitch = tpitch;
	a.nsets = nsets; a.qmod = sg.qmod; a.tdiv = sg.tdiv; a.dim = dim; a.K = K; a.countThresh = count_thresh;
	a.qblk = q->block_rows; a.qbpitch = (size_t)q->block_pitch_rows; a.tblk = t->block_rows; a.tbpitch = (size_t)t->block_pitch_rows;
	a.toff = sg.toff; a.tmod = sg.tmod;
	const size_t outRows = (size_t)nsets * q->n;
	const int qTiles = (q->n + 255) / 256;
	// Train-range splits only where the (set, query tile) grid alone cannot fill the chip (a single keyframe pair: 12 workgroups).  From kFillBlocks
	// workgroups on (2 per CU) every workgroup walks its whole train set: no partial lists, no merge pass (their HBM traffic was 16x the algorithmic bytes).
	static const int kTargetBlocks = getenv("MCS_MATCH_BLOCKS") ? atoi(getenv("MCS_MATCH_BLOCKS")) : 2048;
	static const int kFillBlocks = getenv("MCS_MATCH_FILL") ? atoi(getenv("MCS_MATCH_FILL")) : 512;
	int splits = (long long)qTiles * nsets >= kFillBlocks ? 1 : (int)((kTargetBlocks + (long long)qTiles * nsets - 1) / ((long long)qTiles * nsets));
	splits = std::max(1, std::min(splits, (t->n + 255) / 256));
	a.splits = splits;
	if (splits > 1) {
		HIPCHK(c->partial.reserve(outRows * splits * K * sizeof(uint32_t)));
		HIPCHK(c->partialCount.reserve(outRows * splits * sizeof(int)));
	}
	a.partial = c->partial.as<uint32_t>(); a.partialCount = c->partialCount.as<int>();
	a.outDist = outDist; a.outIdx = outIdx; a.outCount = outCount;
	if (match_mfma_shape(a) && t->n > 0) {
		// the matrix-core matcher reads train sets that one pass has compacted and expanded (256 bytes per masked 32-byte row); beyond kExpandCap the v_bcnt kernel serves
		static const size_t kExpandCap = getenv("MCS_MATCH_EXPAND_MB") ? (size_t)atoll(getenv("MCS_MATCH_EXPAND_MB")) << 20 : (size_t)8 << 30;
		size_t bA = 0, bW = 0;
		match_mfma_scratch(a, sg.nt_sets, &bA, &bW, &a.exStages);
		if (bA <= kExpandCap) {
			HIPCHK(c->exA.reserve(bA)); HIPCHK(c->exW.reserve(bW)); HIPCHK(c->exRows.reserve((size_t)sg.nt_sets * sizeof(int)));
			a.exA = c->exA.as<uint4>(); a.exW = c->exW.as<float>(); a.exRows = c->exRows.as<int>(); a.tsets = sg.nt_sets;
		}
	}
	c->tic("match");
	static const bool valuOnly = getenv("MCS_MATCH_VALU") != nullptr;
	if (deferred) {
		if (!valuOnly && match_mfma_serves(a)) {
			// the previous deferred search's LISTS (other stream) may still read the expanded sets: order the pass behind them (in a pipelined caller they finished long ago)
			if (c->searchSeq > 0) HIPCHK(hipStreamWaitEvent(c->stream, c->evLists, 0));
			launch_match_expand(a, c->stream); a.exDone = 1;
		}
		HIPCHK(hipEventRecord(c->evMatch, c->stream));
		HIPCHK(hipStreamWaitEvent(ls, c->evMatch, 0));
		if (c->searchSeq > 1) HIPCHK(hipStreamWaitEvent(ls, c->evGreedyBuf[slot], 0));   // the greedy pass that read this list buffer (two searches ago)
	}
	launch_match(a, ls);
	if (deferred) HIPCHK(hipEventRecord(c->evLists, ls));
	c->toc("match");
	HIPCHK(hipGetLastError());
	return MCS_OK;
}

extern "C" {

int mcs_match_topk_batched(mcs_ctx* c, int nsets, const mcs_desc_set* q, size_t qpitch, const mcs_desc_set* t, size_t tpitch, int dim, int K,
                           int count_thresh, mcs_mem_kind kind, int32_t* out_dist, int32_t* out_idx, int32_t* out_count_le) {
	if (int r = validate_sets(c, nsets, q, t, dim, K)) return r;
	if (!out_dist || !out_idx || !out_count_le) return fail(MCS_ERR_INVALID, "null output");
	if (q->n == 0) return MCS_OK;
	HIPCHK(hipSetDevice(c->device));
	DevSets d{};
	const SetGrid sg = grid_batched(nsets, qpitch, tpitch);
	Staging st(c, kind == MCS_MEM_HOST);
	if (int r = stage_sets(st, sg, q, qpitch, t, tpitch, &d, nullptr, nullptr, nullptr, 0)) return r;
	const size_t outRows = (size_t)nsets * q->n;
	int *dDist = nullptr, *dIdx = nullptr, *dCount = nullptr;
	st.out(&dDist, out_dist, outRows * K * 4); st.out(&dIdx, out_idx, outRows * K * 4); st.out(&dCount, out_count_le, outRows * 4);
	if (int r = st.commit()) return r;
	d.resolve();
	return st.finish(run_topk(c, d, sg, q, qpitch, t, tpitch, dim, K, count_thresh, 0x7FFFFFFF, dDist, dIdx, dCount));
}

int mcs_match_topk(mcs_ctx* c, const mcs_desc_set* q, const mcs_desc_set* t, int dim, int K, int count_thresh, mcs_mem_kind kind,
                   int32_t* out_dist, int32_t* out_idx, int32_t* out_count_le) {
	return mcs_match_topk_batched(c, 1, q, 0, t, 0, dim, K, count_thresh, kind, out_dist, out_idx, out_count_le);
}

// mode 0: SearchByBoW(KF,KF)   1: SearchByBoW(KF,F)   2: SearchForTriangulationRaw
static int search_common(mcs_ctx* c, int mode, const SetGrid& sg, const mcs_desc_set* q, size_t qpitch, const mcs_desc_set* t, size_t tpitch, int dim,
                         double nnratio, int K, mcs_mem_kind kind, const double* rays1, const double* rays2, const double* E, size_t Epitch, int nrCams,
                         int32_t* out_match, int32_t* out_nmatches, int32_t* out_fallbacks) {
	const int nsets = sg.nsets;
	if (sg.nq_sets < 1 || sg.nt_sets < 1) return fail(MCS_ERR_INVALID, "bad set count");
	if (int r = validate_sets(c, nsets, q, t, dim, K)) return r;
	if (!out_match || !out_nmatches) return fail(MCS_ERR_INVALID, "null output");
	if (t->n > 131072) return fail(MCS_ERR_UNSUPPORTED, "more than 131072 train rows per set");
	if (mode == 2 && (!rays1 || !rays2 || !E || nrCams < 1)) return fail(MCS_ERR_INVALID, "triangulation search needs rays and essential matrices");
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	// Deferred form (mcs_ctx_set_async_search, device memory): lists AND greedy pass run on the greedy stream, ordered behind the inputs by an event and
	// behind the previous search by the stream itself; the caller's stream goes on at once (the next batch's extraction fills the matcher's stalls).
	const bool deferred = kind == MCS_MEM_DEVICE && c->overlap() && c->asyncSearch;
	if (deferred) {
		if (q->n == 0) { HIPCHK(hipEventRecord(c->evMatch, s)); HIPCHK(hipStreamWaitEvent(c->side2, c->evMatch, 0)); }   // otherwise in run_topk
	} else if (int r = ctx_join_greedy(c, s)) return r;   // the previous search's greedy pass (side stream) still reads the shared list buffers
	const bool havingMasks = q->mask != nullptr;
	// thresholds of cORBmatcher::cORBmatcher (src/cORBmatcher.cpp:46-65); only TH_LOW_ is used by these three searches
	const int thLow = havingMasks ? (int)floor((double)dim) : 2 * dim;
	DevSets d{};
	Staging st(c, kind == MCS_MEM_HOST);
	if (int r = stage_sets(st, sg, q, qpitch, t, tpitch, &d, mode == 2 ? &rays1 : nullptr, mode == 2 ? &rays2 : nullptr,
	                       mode == 2 ? &E : nullptr, Epitch * (size_t)(nsets - 1) + (size_t)nrCams * nrCams * 9)) return r;
	const size_t rows = (size_t)nsets * q->n, outN = (size_t)nsets * (mode == 1 ? t->n : q->n);
	GreedyArgs g{};
	st.out(&g.outMatch, out_match, outN * 4); st.out(&g.outCount, out_nmatches, (size_t)nsets * 4); st.out(&g.outFallbacks, out_fallbacks, (size_t)nsets * 4);
	if (int r = st.commit()) return r;   // (a device-kind search declares nothing: no claim, no wait)
	d.resolve();
	// deferred: two list buffers in turn, the greedy pass on a stream of its own — it is a chain of dependent round trips with a few waves per CU, the matcher waits
	// 45 % of its cycles: side by side (greedy pass of search n, lists of search n + 1) the greedy pass disappears from the matcher stream's critical path
	const int slot = deferred ? (int)(c->searchSeq & 1) : 0;
	HIPCHK(c->topCnt.reserve(std::max<size_t>(rows, 1) * 4));
	{
		// Rows that can never influence a decision stay out of the lists: SearchByBoW needs best <= TH_LOW and, for the ratio
		// test, seconds up to the largest d with nnratio*d <= TH_LOW (any farther second passes best < nnratio*second for every
		// admissible best); SearchForTriangulationRaw only collects dist <= TH_LOW (:1062).
		int maxDist = thLow;
		if (mode != 2) while (maxDist < 8 * dim && nnratio * static_cast<double>(maxDist + 1) <= static_cast<double>(thLow)) ++maxDist;
		if (q->n > 0)
			if (int r = run_topk(c, d, sg, q, qpitch, t, tpitch, dim, K, -1, maxDist, nullptr, nullptr, c->topCnt.as<int>(), deferred ? c->side2 : nullptr, slot)) return r;
	}
	g.qd = d.qd; g.qm = d.qm; g.qvalid = d.qvalid; g.qgroup = d.qgroup; g.td = d.td; g.tm = d.tm; g.tvalid = d.tvalid; g.tgroup = d.tgroup;
	g.nq = q->n; g.nt = t->n; g.qstride = q->stride; g.tstride = t->stride; g.qpitch = qpitch; g.tpitch = tpitch;
	g.nsets = nsets; g.qmod = sg.qmod; g.tdiv = sg.tdiv; g.dim = dim; g.K = K; g.keys = (slot ? c->topKeys2 : c->topKeys).as<uint32_t>();
	g.qblk = q->block_rows; g.qbpitch = (size_t)q->block_pitch_rows; g.tblk = t->block_rows; g.tbpitch = (size_t)t->block_pitch_rows;
	g.toff = sg.toff; g.tmod = sg.tmod;
	g.thLow = thLow; g.thInclusive = mode == 1 ? 1 : 0; g.ratio = nnratio; g.mode = mode;
	g.rays1 = rays1; g.rays2 = rays2; g.E = E; g.Epitch = Epitch; g.nrCams = nrCams;
	{ static const int ms = getenv("MCS_JACOBI_MAX_SWEEPS") ? atoi(getenv("MCS_JACOBI_MAX_SWEEPS")) : 0; g.jacMaxSweeps = ms; }
	if (kind == MCS_MEM_DEVICE) {
		if (deferred) {
			if (q->n > 0) HIPCHK(hipStreamWaitEvent(c->side3, c->evLists, 0));
			else HIPCHK(hipStreamWaitEvent(c->side3, c->evMatch, 0));
			launch_greedy(g, c->side3);
			HIPCHK(hipEventRecord(c->evGreedyBuf[slot], c->side3));
			HIPCHK(hipEventRecord(c->evGreedy, c->side3));
			HIPCHK(hipEventRecord(c->evSearch[c->searchSeq & 3], c->side3));
			++c->searchSeq;
			c->greedyPending = true;
			c->lastResultStream = c->side3;
		} else if (c->overlap()) {
			// the greedy resolution is one wave per set pair (latency-bound): run it on the side stream so that whatever the caller
			// enqueues next on the main stream (the next batch's extraction) fills the idle CUs.  mcs_ctx_join / the next search /
			// mcs_ctx_synchronize order later work behind it.
			HIPCHK(hipEventRecord(c->evMatch, s));
			HIPCHK(hipStreamWaitEvent(c->side2, c->evMatch, 0));
			launch_greedy(g, c->side2);
			HIPCHK(hipEventRecord(c->evGreedy, c->side2));
			c->greedyPending = true;
			c->lastResultStream = c->side2;
		} else { c->tic("greedy"); launch_greedy(g, s); c->toc("greedy"); c->lastResultStream = s; }
		HIPCHK(hipGetLastError());
		return MCS_OK;
	}
	c->tic("greedy"); launch_greedy(g, s); c->toc("greedy");
	HIPCHK(hipGetLastError());
	// page-locked outputs: one launch instead of three copies (mcs_host.h device_view)
	static const bool outKernel = !(getenv("MCS_OUT_KERNEL") && atoi(getenv("MCS_OUT_KERNEL")) == 0);
	int* dm = (int*)device_view(out_match); int* dn = (int*)device_view(out_nmatches); int* df = (int*)device_view(out_fallbacks);
	const bool viaKernel = outKernel && dm && dn && (df || !out_fallbacks);
	if (viaKernel) {
		launch_search_out(dm, g.outMatch, outN, dn, g.outCount, df, g.outFallbacks, nsets, s);
		HIPCHK(hipGetLastError());
	}
	return st.finish(MCS_OK, !viaKernel);
}

int mcs_search_kf_kf(mcs_ctx* c, int nsets, const mcs_desc_set* kf1, size_t pitch1, const mcs_desc_set* kf2, size_t pitch2, int dim, double nnratio,
                     int K, mcs_mem_kind kind, int32_t* match12, int32_t* nmatches, int32_t* fallbacks) {
	return search_common(c, 0, grid_batched(nsets, pitch1, pitch2), kf1, pitch1, kf2, pitch2, dim, nnratio, K, kind, nullptr, nullptr, nullptr, 0, 0, match12, nmatches, fallbacks);
}

int mcs_search_kf_kf_ring(mcs_ctx* c, int nframes_total, int first, int count, const mcs_desc_set* frames, size_t pitch_rows, int dim, double nnratio, int K,
                          mcs_mem_kind kind, int32_t* match12, int32_t* nmatches, int32_t* fallbacks) {
	if (nframes_total < 2 || first < 0 || count < 1 || first + count > nframes_total) return fail(MCS_ERR_INVALID, "bad ring range");
	if (kind != MCS_MEM_DEVICE) return fail(MCS_ERR_UNSUPPORTED, "the ring form takes device memory");
	if (!frames) return fail(MCS_ERR_INVALID, "null argument");
	// the query side starts at frame `first`: shift its pointers, the train side stays at frame 0 and is addressed through (first + s - 1) mod total
	mcs_desc_set q = *frames;
	const size_t shift = (size_t)first * pitch_rows;
	q.desc += shift * frames->stride;
	if (q.mask) q.mask += shift * frames->stride;
	if (q.valid) q.valid += shift;
	if (q.group) q.group += shift;
	return search_common(c, 0, grid_ring(nframes_total, first, count), &q, pitch_rows, frames, pitch_rows, dim, nnratio, K, kind, nullptr, nullptr, nullptr, 0, 0, match12, nmatches, fallbacks);
}

int mcs_search_kf_f(mcs_ctx* c, int nsets, const mcs_desc_set* kf, size_t pitchKF, const mcs_desc_set* f, size_t pitchF, int dim, double nnratio, int K,
                    mcs_mem_kind kind, int32_t* matchF, int32_t* nmatches, int32_t* fallbacks) {
	return search_common(c, 1, grid_batched(nsets, pitchKF, pitchF), kf, pitchKF, f, pitchF, dim, nnratio, K, kind, nullptr, nullptr, nullptr, 0, 0, matchF, nmatches, fallbacks);
}

int mcs_search_kf_f_sweep(mcs_ctx* c, int nkf, const mcs_desc_set* kf, size_t pitchKF, int nframes, const mcs_desc_set* f, size_t pitchF, int dim,
                          double nnratio, int K, mcs_mem_kind kind, int32_t* matchF, int32_t* nmatches, int32_t* fallbacks) {
	if (nkf < 1 || nframes < 1 || (long long)nkf * nframes > (1 << 24)) return fail(MCS_ERR_INVALID, "bad keyframe / frame count");
	auto rows_of = [](const mcs_desc_set* d) { return (size_t)(d ? (d->block_rows ? d->block_rows : d->n) : 0); };   // interleaved blocks: only a block must fit
	if ((nkf > 1 && pitchKF < rows_of(kf)) || (nframes > 1 && pitchF < rows_of(f))) return fail(MCS_ERR_INVALID, "set pitch smaller than the set");
	return search_common(c, 1, grid_sweep(nkf, nframes), kf, pitchKF, f, pitchF, dim, nnratio, K, kind, nullptr, nullptr, nullptr, 0, 0, matchF, nmatches, fallbacks);
}

int mcs_search_triangulation(mcs_ctx* c, int nsets, const mcs_desc_set* kf1, size_t pitch1, const mcs_desc_set* kf2, size_t pitch2, const double* rays1,
                             const double* rays2, const double* E, int nrCams, int dim, int K, mcs_mem_kind kind, int32_t* match12,
                             int32_t* nmatches, int32_t* fallbacks) {
	return search_common(c, 2, grid_batched(nsets, pitch1, pitch2), kf1, pitch1, kf2, pitch2, dim, 0.0, K, kind, rays1, rays2, E, 0, nrCams, match12, nmatches, fallbacks);
}

int mcs_search_triangulation_sweep(mcs_ctx* c, int nsets, const mcs_desc_set* kf1, size_t pitch1, const mcs_desc_set* kf2, size_t pitch2, const double* rays1,
                                   const double* rays2, const double* E, size_t E_set_pitch, int nrCams, int dim, int K, mcs_mem_kind kind,
                                   int32_t* match12, int32_t* nmatches, int32_t* fallbacks) {
	if (E_set_pitch != 0 && E_set_pitch < (size_t)nrCams * nrCams * 9) return fail(MCS_ERR_INVALID, "E_set_pitch smaller than one block of essential matrices");
	return search_common(c, 2, grid_batched(nsets, pitch1, pitch2), kf1, pitch1, kf2, pitch2, dim, 0.0, K, kind, rays1, rays2, E, E_set_pitch, nrCams, match12, nmatches, fallbacks);
}

int mcs_rows_valid(mcs_ctx* c, const int32_t* nkp_dev, int nimg, int cap, uint8_t* valid_dev) {
	if (!c || !nkp_dev || !valid_dev || nimg < 1 || cap < 1) return fail(MCS_ERR_INVALID, "bad argument");
	HIPCHK(hipSetDevice(c->device));
	launch_rows_valid(nkp_dev, nimg, cap, valid_dev, c->stream);
	HIPCHK(hipGetLastError());
	return MCS_OK;
}

int mcs_rig_pack_headers(mcs_ctx* c, const int32_t* nkp_dev, int nimg, int cap, uint8_t* blocks_dev, int row_stride) {
	if (!c || !nkp_dev || !blocks_dev || nimg < 1 || cap < 1 || row_stride < 4 || (row_stride & 3)) return fail(MCS_ERR_INVALID, "bad argument");
	HIPCHK(hipSetDevice(c->device));
	launch_rig_pack_headers(nkp_dev, nimg, cap, blocks_dev, row_stride, c->stream);
	HIPCHK(hipGetLastError());
	return MCS_OK;
}

int mcs_rig_rows_valid(mcs_ctx* c, const uint8_t* blocks_dev, int nimg, int cap, int row_stride, uint8_t* valid_dev, int32_t* nkp_out_dev) {
	if (!c || !blocks_dev || !valid_dev || nimg < 1 || cap < 1 || row_stride < 4 || (row_stride & 3)) return fail(MCS_ERR_INVALID, "bad argument");
	HIPCHK(hipSetDevice(c->device));
	launch_rig_rows_valid(blocks_dev, nimg, cap, row_stride, valid_dev, nkp_out_dev, c->stream);
	HIPCHK(hipGetLastError());
	return MCS_OK;
}

static int single_distance(mcs_ctx* c, const uint8_t* a, const uint8_t* b, const uint8_t* ma, const uint8_t* mb, int dim, int* out) {
	if (!c || !a || !b || !out || (dim != 16 && dim != 32 && dim != 64)) return fail(MCS_ERR_INVALID, "bad argument");
	HIPCHK(hipSetDevice(c->device));
	Staging st(c, true);
	const uint8_t *da = nullptr, *db = nullptr, *dma = nullptr, *dmb = nullptr; int* dOut = nullptr;
	st.in(&da, a, dim); st.in(&db, b, dim); st.in(&dma, ma, dim); st.in(&dmb, ma ? mb : nullptr, dim); st.out(&dOut, out, sizeof(int));
	if (int r = st.commit()) return r;
	launch_single_distance(da, db, dma, dmb, dim, dOut, c->stream);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_descriptor_distance(mcs_ctx* c, const uint8_t* a, const uint8_t* b, int dim, int* out) { return single_distance(c, a, b, nullptr, nullptr, dim, out); }
int mcs_descriptor_distance_masked(mcs_ctx* c, const uint8_t* a, const uint8_t* b, const uint8_t* ma, const uint8_t* mb, int dim, int* out) {
	if (!ma || !mb) return fail(MCS_ERR_INVALID, "null masks");
	return single_distance(c, a, b, ma, mb, dim, out);
}

int mcs_distinctive_descriptors(mcs_ctx* c, const uint8_t* desc, const uint8_t* mask, int stride, int dim, const int32_t* offsets, int npoints,
                                mcs_mem_kind kind, int32_t* best_idx) {
	if (!c || !desc || !offsets || !best_idx) return fail(MCS_ERR_INVALID, "null argument");
	if (dim != 16 && dim != 32 && dim != 64) return fail(MCS_ERR_INVALID, "dim must be 16, 32 or 64");
	if (stride < dim || (stride & 3) || npoints < 0) return fail(MCS_ERR_INVALID, "bad stride / count");
	if (npoints == 0) return MCS_OK;
	size_t rows = 0;
	if (kind == MCS_MEM_HOST) {   // (device kind: offsets are validated by the caller, and nothing is staged)
		if (offsets[0] != 0) return fail(MCS_ERR_INVALID, "offsets[0] must be 0");
		for (int k = 0; k < npoints; ++k)
			if (offsets[k + 1] < offsets[k] || offsets[k + 1] - offsets[k] > 65535) return fail(MCS_ERR_INVALID, "offsets must be non-decreasing, <= 65535 rows per map point");
		rows = (size_t)offsets[npoints];
	}
	HIPCHK(hipSetDevice(c->device));
	DistinctArgs a{};
	a.stride = stride; a.dim = dim; a.npoints = npoints;
	Staging st(c, kind == MCS_MEM_HOST);
	st.in(&a.desc, desc, rows * stride); st.in(&a.mask, mask, rows * stride); st.in(&a.offsets, offsets, ((size_t)npoints + 1) * 4);
	st.out(&a.bestIdx, best_idx, (size_t)npoints * 4);
	if (int r = st.commit()) return r;
	launch_distinct(a, c->stream);
	HIPCHK(hipGetLastError());
	return st.finish(MCS_OK);
}

int mcs_selftest_shared_reciprocal(mcs_ctx* c, uint64_t seed, int n, int32_t* mismatches) {
	if (!c || !mismatches || n < 1) return fail(MCS_ERR_INVALID, "bad argument");
	HIPCHK(hipSetDevice(c->device));
	int* d = nullptr;
	Staging st(c, true);
	st.download(&d, mismatches, 4);
	if (int r = st.commit()) return r;
	(void)hipMemsetAsync(d, 0, 4, c->stream);
	launch_selftest_recip(seed, n, d, c->stream);
	const bool launched = hipGetLastError() == hipSuccess;
	if (st.finish(launched ? MCS_OK : MCS_ERR_HIP) != MCS_OK) return fail(MCS_ERR_HIP, "selftest kernel failed");
	return MCS_OK;
}

}  // extern "C"
