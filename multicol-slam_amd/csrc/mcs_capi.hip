// mcs_capi.hip — C ABI (include/mcs_c.h) of libmcs_hip.so: errors, contexts (streams, timers), construction and release of extractors.  The rest of the
// extractor's ABI: mcs_extract.hip (batches, taps), mcs_ties.hip (rounding ties), mcs_gtable.hip (the fast pass's tables); the matcher's: mcs_capi_match.hip.
// There is no CPU fallback in this library: every entry point needs a HIP device.
#include "mcs_extractor.h"
#include "mcs_plan.h"

#include <cstdio>
#include <cstdlib>

namespace mcs {
bool upload_describe_tables(const signed char* pattern);
const signed char kPattern[2048] = {
#include "learned_pattern_64_orb.inc"
};
}  // namespace mcs

using namespace mcs;

std::string& mcs_err() { static thread_local std::string e; return e; }

// Everything mcs_extractor_create does after `new`: device tables, buffers, uploads.  On any failure the caller releases the half-built object through
// mcs_extractor_destroy (every pointer starts out null).
static int extractor_build(mcs_extractor* e, const ExtractPlan& plan) {
	const PyrDesc& hd = e->hd;
	if (!upload_describe_tables(kPattern)) return fail(MCS_ERR_HIP, "pattern tables: upload failed (or the distinct-point rounds of mcs_describe.hip do not fit this pattern)");
	const size_t B = e->maxBatch;
#define ALLOC(ptr, bytes) do { hipError_t _e = hipMalloc((void**)&(ptr), (bytes)); if (_e != hipSuccess) return fail(MCS_ERR_HIP, std::string("hipMalloc ") + #ptr + ": " + hipGetErrorString(_e)); } while (0)
	ALLOC(e->d_desc, sizeof(PyrDesc));
	ALLOC(e->d_cells, sizeof(CellInfo) * e->cells.size());
	ALLOC(e->d_taps, sizeof(ResizeTap) * std::max<size_t>(plan.taps.size(), 1));
	ALLOC(e->d_maskMap, sizeof(short) * plan.maps.size());
	ALLOC(e->d_pyr, B * hd.pyrBytes);
	ALLOC(e->d_blur, B * hd.pyrBytes);
	ALLOC(e->d_slots, B * hd.slotsPerImage * sizeof(uint32_t));
	ALLOC(e->d_dense, B * hd.densePerImage * sizeof(uint32_t));
	ALLOC(e->d_knode, B * hd.densePerImage * sizeof(unsigned short));
	ALLOC(e->d_sel, B * hd.selPerImage * sizeof(uint32_t));
	ALLOC(e->d_selAngle, B * hd.selPerImage * sizeof(float));
	ALLOC(e->d_cellCount, B * hd.cellsPerImage * sizeof(int));
	ALLOC(e->d_denseCount, B * hd.nlevels * sizeof(int));
	ALLOC(e->d_selCount, B * hd.nlevels * sizeof(int));
	ALLOC(e->d_status, sizeof(int));
	ALLOC(e->d_cams, B * sizeof(OcamDev));
	const size_t slotsPerImage = (size_t)kp_slots_per_image(hd);
	ALLOC(e->d_fbCount, 3 * sizeof(int));   // [0] fallback list, [1] pre-list, [2] tie list
	if (hipHostMalloc((void**)&e->h_status, 2 * sizeof(int), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); e->h_status = nullptr; }   // (without it host-kind outputs take the runtime's copies)
	ALLOC(e->d_tieList, B * slotsPerImage * sizeof(uint32_t));
	ALLOC(e->d_fbList, B * slotsPerImage * sizeof(uint32_t));
	ALLOC(e->d_preList, B * slotsPerImage * sizeof(uint32_t));
	ALLOC(e->d_fbStats, 2 * sizeof(unsigned long long));   // [0] exact-pass keypoints, [1] tie-listed keypoints
	ALLOC(e->d_tieMin, sizeof(unsigned long long));
	ALLOC(e->d_aux, B * slotsPerImage * describe_aux_bytes());
	ALLOC(e->d_gTab, B * (size_t)kGDevDoubles * sizeof(double));
	ALLOC(e->d_nkp, B * sizeof(int));
	ALLOC(e->d_kps, B * hd.kpCap * sizeof(mcs_keypoint));
	ALLOC(e->d_odesc, B * hd.kpCap * (size_t)hd.descSize);
	ALLOC(e->d_omask, B * hd.kpCap * (size_t)hd.descSize);
	ALLOC(e->d_rays, B * hd.kpCap * 3 * sizeof(double));
#undef ALLOC
	HIPCHK(hipMemcpy(e->d_desc, &hd, sizeof(PyrDesc), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(e->d_cells, e->cells.data(), sizeof(CellInfo) * e->cells.size(), hipMemcpyHostToDevice));
	if (!plan.taps.empty()) HIPCHK(hipMemcpy(e->d_taps, plan.taps.data(), sizeof(ResizeTap) * plan.taps.size(), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(e->d_maskMap, plan.maps.data(), sizeof(short) * plan.maps.size(), hipMemcpyHostToDevice));
	HIPCHK(hipMemset(e->d_status, 0, sizeof(int)));
	HIPCHK(hipMemset(e->d_fbCount, 0, 3 * sizeof(int)));
	HIPCHK(hipMemset(e->d_fbStats, 0, 2 * sizeof(unsigned long long)));
	{ const unsigned long long inf = 0x7FF0000000000000ull; HIPCHK(hipMemcpy(e->d_tieMin, &inf, sizeof(inf), hipMemcpyHostToDevice)); }   // +inf: no coordinate seen yet
	if (hipHostMalloc((void**)&e->hostTie.host, sizeof(TieCaptureHeader) + (size_t)kHostTieSlots * sizeof(TieCaptureEntry), hipHostMallocDefault) == hipSuccess) {
		memset(e->hostTie.host, 0, sizeof(TieCaptureHeader));
		e->hostTie.dev = (uint8_t*)device_view(e->hostTie.host);
	} else { (void)hipGetLastError(); e->hostTie.host = nullptr; }   // (without it host-kind batches take the whole-level download)
	if (getenv("MCS_DESCRIBE_EXACT")) e->describeMode = 1;   // A/B and debugging: the exact pass for every keypoint
	HIPCHK(hipMemset(e->d_pyr, 0, B * hd.pyrBytes));
	HIPCHK(hipMemset(e->d_blur, 0, B * hd.pyrBytes));
	return MCS_OK;
}

extern "C" {

const char* mcs_last_error(void) { return mcs_err().c_str(); }
int mcs_abi_version(void) { return MCS_ABI_VERSION; }

int mcs_device_count(int* n) {
	if (!n) return fail(MCS_ERR_INVALID, "null");
	HIPCHK(hipGetDeviceCount(n));
	return MCS_OK;
}

int mcs_ctx_create(int device, void* hip_stream, mcs_ctx** out) {
	if (!out) return fail(MCS_ERR_INVALID, "out is null");
	int n = 0;
	HIPCHK(hipGetDeviceCount(&n));
	if (n <= 0 || device < 0 || device >= n) return fail(MCS_ERR_HIP, "no usable HIP device (libmcs_hip has no CPU fallback)");
	HIPCHK(hipSetDevice(device));
	mcs_ctx* c = new mcs_ctx;
	c->device = device;
	if (hip_stream) c->stream = (hipStream_t)hip_stream;
	else { HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->ownStream = true; }
	if (getenv("MCS_NO_OVERLAP") == nullptr) {
		// (stream priorities — resize chain urgent, deferred matcher least urgent or most urgent, and every other combination — change nothing measurable)
		HIPCHK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
		// A/B: MCS_MATCH_CU_MASK=<hex word> confines the deferred matcher's stream (MCS_GREEDY_CU_MASK: the greedy pass's) to the CUs whose bit is set in the word,
		// repeated over the chip's CUs — its workgroups (3 waves per SIMD at 168 registers) otherwise leave no room for anybody else on the CUs they hold
		auto masked = [&](hipStream_t* st, const char* var) -> hipError_t {
			const char* m = getenv(var);
			if (!m || !*m) return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
			char* end = nullptr;
			const unsigned long v = strtoul(m, &end, 16);
			if (end == m || *end != '\0' || v == 0 || v > 0xFFFFFFFFul) { fprintf(stderr, "mcs: %s=\"%s\" is not a non-zero 32-bit hex word\n", var, m); return hipErrorInvalidValue; }
			// NOTE: hipExtStreamCreateWithCUMask makes a BLOCKING stream (it synchronises implicitly with the null stream), unlike the hipStreamNonBlocking ones of
			// the default path: an A/B through these switches changes more than CU placement
			uint32_t words[16];
			for (auto& w : words) w = (uint32_t)v;
			hipDeviceProp_t prop;
			if (hipGetDeviceProperties(&prop, device) != hipSuccess) return hipErrorInvalidValue;
			return hipExtStreamCreateWithCUMask(st, (uint32_t)((prop.multiProcessorCount + 31) / 32), words);
		};
		HIPCHK(masked(&c->side2, "MCS_MATCH_CU_MASK"));
		HIPCHK(masked(&c->side3, "MCS_GREEDY_CU_MASK"));
		HIPCHK(hipEventCreateWithFlags(&c->evLists, hipEventDisableTiming));
		for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreateWithFlags(&c->evGreedyBuf[i], hipEventDisableTiming));

		HIPCHK(hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&c->evPyr, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&c->evBlur, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&c->evMatch, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&c->evGreedy, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&c->evDescFork, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&c->evDescJoin, hipEventDisableTiming));

		for (int i = 0; i < 4; ++i) HIPCHK(hipEventCreateWithFlags(&c->evSearch[i], hipEventDisableTiming));
	}
	*out = c;
	return MCS_OK;
}

// make the context's main stream wait for everything queued on the side stream (outputs of the searches are written there)
int mcs_ctx_join(mcs_ctx* c) {
	if (!c) return fail(MCS_ERR_INVALID, "null ctx");
	return ctx_join_greedy(c, c->stream);
}

int mcs_ctx_set_async_search(mcs_ctx* c, int on) {
	if (!c) return fail(MCS_ERR_INVALID, "null ctx");
	HIPCHK(hipStreamSynchronize(c->stream));
	if (c->side2) { HIPCHK(hipStreamSynchronize(c->side2)); HIPCHK(hipStreamSynchronize(c->side3)); }
	const bool was = c->asyncSearch;
	c->asyncSearch = on != 0 && c->side2 != nullptr;
	if (was != c->asyncSearch) { c->upload = nullptr; c->lastResultStream = nullptr; }   // the transfer stream is re-scored for the new mode (mcs_copy.hip); the result stream follows the next search
	return MCS_OK;
}

int mcs_ctx_search_fence(mcs_ctx* c, int lag) {
	if (!c || lag < 0 || lag > 2) return fail(MCS_ERR_INVALID, "lag must be 0, 1 or 2");
	if (!c->asyncSearch) return lag == 0 ? mcs_ctx_join(c) : MCS_OK;   // in-order searches: only the latest greedy pass can still be running
	const long long want = c->searchSeq - 1 - lag;
	if (want >= 0) HIPCHK(hipStreamWaitEvent(c->stream, c->evSearch[want & 3], 0));
	if (lag == 0) c->greedyPending = false;
	return MCS_OK;
}

int mcs_ctx_destroy(mcs_ctx* c) {
	if (!c) return MCS_OK;
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	while (!c->extractors.empty()) (void)mcs_extractor_destroy(c->extractors.back());   // an extractor must not outlive the stream it runs on
	for (auto& kv : c->timers) { if (kv.second.a) { (void)hipEventDestroy(kv.second.a); (void)hipEventDestroy(kv.second.b); } }
	if (c->side) {
		(void)hipStreamSynchronize(c->side);
		(void)hipStreamSynchronize(c->side2);
		(void)hipStreamDestroy(c->side2);
		(void)hipStreamSynchronize(c->side3); (void)hipStreamDestroy(c->side3);
		(void)hipEventDestroy(c->evLists); (void)hipEventDestroy(c->evGreedyBuf[0]); (void)hipEventDestroy(c->evGreedyBuf[1]);
		for (int i = 0; i < 4; ++i) if (c->evSearch[i]) (void)hipEventDestroy(c->evSearch[i]);
		(void)hipEventDestroy(c->evFork); (void)hipEventDestroy(c->evPyr); (void)hipEventDestroy(c->evBlur); (void)hipEventDestroy(c->evMatch); (void)hipEventDestroy(c->evGreedy);
		(void)hipEventDestroy(c->evDescFork); (void)hipEventDestroy(c->evDescJoin);
		(void)hipStreamDestroy(c->side);
	}
	for (hipStream_t ps : c->probed) { (void)hipStreamSynchronize(ps); (void)hipStreamDestroy(ps); }
	if (c->ownStream) (void)hipStreamDestroy(c->stream);
	delete c;   // frees the context's device buffers and the mirror (mcs_host.h)
	return MCS_OK;
}

int mcs_ctx_synchronize(mcs_ctx* c) {
	if (!c) return fail(MCS_ERR_INVALID, "null ctx");
	HIPCHK(hipStreamSynchronize(c->stream));
	if (c->side) { HIPCHK(hipStreamSynchronize(c->side)); HIPCHK(hipStreamSynchronize(c->side2)); HIPCHK(hipStreamSynchronize(c->side3)); c->greedyPending = false; }
	return MCS_OK;
}

int mcs_ctx_enable_timing(mcs_ctx* c, int on) {
	if (!c) return fail(MCS_ERR_INVALID, "null ctx");
	if (c->timing != (on != 0)) c->lastResultStream = nullptr;   // per-kernel timing runs the searches in order on the main stream: what the last search recorded belongs to the other mode
	c->timing = on != 0;
	return MCS_OK;
}

int mcs_ctx_kernel_ms(mcs_ctx* c, const char* name, float* ms) {
	if (!c || !name || !ms) return fail(MCS_ERR_INVALID, "null");
	auto it = c->timers.find(name);
	if (it == c->timers.end() || !it->second.used) return fail(MCS_ERR_INVALID, std::string("no timing for ") + name);
	HIPCHK(hipEventSynchronize(it->second.b));
	HIPCHK(hipEventElapsedTime(ms, it->second.a, it->second.b));
	return MCS_OK;
}

// ------------------------------------------------------------------------------------------------ extractor
// check, plan (mcs_plan.hip: no device needed), new, then allocate and upload (extractor_build) with ONE release path behind `new`
int mcs_extractor_create(mcs_ctx* ctx, const mcs_extractor_params* p, int width, int height, int max_batch, mcs_extractor** out) {
	if (!ctx || !p || !out) return fail(MCS_ERR_INVALID, "null argument");
	if (p->nlevels < 1 || p->nlevels > MCS_MAX_LEVELS) return fail(MCS_ERR_INVALID, "nlevels out of range");
	if (p->descSize != 16 && p->descSize != 32 && p->descSize != 64) return fail(MCS_ERR_INVALID, "descSize must be 16, 32 or 64");
	if (p->useAgast) {
		if (p->fastAgastType < 0 || p->fastAgastType > 3) return fail(MCS_ERR_INVALID, "fastAgastType must be 0 (AGAST_5_8), 1 (AGAST_7_12d), 2 (AGAST_7_12s) or 3 (OAST_9_16) with useAgast");
		// the device stores "no corner" as score 0 and a corner's score is >= the threshold; cv::AGAST's bisection never returns more than 254
		if (p->fastThreshold < 1 || p->fastThreshold > 254) return fail(MCS_ERR_UNSUPPORTED, "useAgast needs 1 <= fastThreshold <= 254");
	} else if (p->fastAgastType < 0 || p->fastAgastType > 2) return fail(MCS_ERR_INVALID, "fastAgastType must be 0 (TYPE_5_8), 1 (TYPE_7_12) or 2 (TYPE_9_16)");
	if (!(p->scaleFactor > 1.0f)) return fail(MCS_ERR_INVALID, "scaleFactor must be > 1");
	if (max_batch < 1 || width < 1 || height < 1 || p->nfeatures < 1) return fail(MCS_ERR_INVALID, "bad size");
	HIPCHK(hipSetDevice(ctx->device));

	ExtractPlan plan;
	std::string why;
	if (int r = plan_extractor(*p, width, height, &plan, &why)) return fail(r, why);

	mcs_extractor* e = new mcs_extractor;
	e->ctx = ctx; e->params = *p; e->maxBatch = max_batch;
	e->hd = plan.hd; e->cells = std::move(plan.cells);
	if (int r = extractor_build(e, plan)) { (void)mcs_extractor_destroy(e); return r; }
	ctx->extractors.push_back(e);
	*out = e;
	return MCS_OK;
}

int mcs_extractor_destroy(mcs_extractor* e) {
	if (!e) return MCS_OK;
	(void)hipSetDevice(e->ctx->device);
	(void)hipStreamSynchronize(e->ctx->stream);
	{
		std::vector<mcs_extractor*>& v = e->ctx->extractors;
		v.erase(std::remove(v.begin(), v.end(), e), v.end());
	}
	void* ptrs[] = {e->d_desc, e->d_cells, e->d_taps, e->d_maskMap, e->d_pyr, e->d_blur, e->d_slots, e->d_dense, e->d_knode,
	                e->d_sel, e->d_cellCount, e->d_denseCount, e->d_selCount, e->d_status, e->d_cams, e->d_nkp, e->d_kps, e->d_odesc,
	                e->d_omask, e->d_rays, e->d_fbCount, e->d_fbList, e->d_preList, e->d_fbStats, e->d_tieMin, e->d_aux, e->d_gTab, e->d_selAngle, e->d_tieList};
	for (void* p : ptrs) (void)hipFree(p);
	for (mcs_extractor::Graph& g : e->graphs) (void)hipGraphExecDestroy(g.exec);
	(void)hipFree(e->d_resMask);
	if (e->h_status) (void)hipHostFree(e->h_status);
	free_tie_capture(e);
	if (e->hostTie.host) (void)hipHostFree(e->hostTie.host);
	delete e;
	return MCS_OK;
}

int mcs_extractor_kp_capacity(const mcs_extractor* e, int* cap) {
	if (!e || !cap) return fail(MCS_ERR_INVALID, "null");
	*cap = e->hd.kpCap;
	return MCS_OK;
}

int mcs_extractor_levels(const mcs_extractor* e, int* nlevels, int* widths, int* heights, int* features_per_level) {
	if (!e) return fail(MCS_ERR_INVALID, "null");
	if (nlevels) *nlevels = e->hd.nlevels;
	for (int l = 0; l < e->hd.nlevels; ++l) {
		if (widths) widths[l] = e->hd.lv[l].w;
		if (heights) heights[l] = e->hd.lv[l].h;
		if (features_per_level) features_per_level[l] = e->hd.lv[l].nfeat;
	}
	return MCS_OK;
}

}  // extern "C"
