// mcs_extract.hip — one batch through the extractor (mcs_extract_batch / _strided): argument checks, buffer binding, host-input staging, the camera table, the
// launch order (forked, replayed from a hipGraph, or timed), the host-kind epilogue; the extractor's per-batch settings, stage taps and the fast pass's self-test.
#include "mcs_extractor.h"
#include "mcs_tiecap.h"

#include <cstdlib>

namespace mcs {
void launch_selftest_fast_model(const OcamDev* cam, const double* tab, unsigned long long seed, int n, int width, int height, unsigned long long* maxDiff, hipStream_t s);

// Host-kind outputs in ONE launch: when the caller's output arrays are page-locked (mcs_host_alloc / hipHostMalloc: visible to the device), the valid rows of the
// five staging arrays, the counts and the batch's status words are written straight into them.  The five hipMemcpyAsync calls this replaces cost ~15 us each for
// ONE multi-frame (7 us of transfer, 8 of runtime per call), plus two more for the status words: a third of the extraction's latency.
struct ExtractOut { int32_t* nkp; uint32_t* kps; uint32_t* desc; uint32_t* mask; uint32_t* rays; int* status; };
extern "C"   // (the kernel's name in traces and profiles is the plain `k_extract_out`)
__global__ __launch_bounds__(256) void k_extract_out(const int* __restrict__ d_nkp, const uint32_t* __restrict__ kps, const uint32_t* __restrict__ desc, const uint32_t* __restrict__ mask,
                                                     const uint32_t* __restrict__ rays, const int* __restrict__ d_status, const int* __restrict__ d_ties, ExtractOut o, int kpCap, int descDw,
                                                     ExtractBuffers b, int nimg, int wavesPerImage, int maxTies, uint8_t* __restrict__ tieOut) {
	if ((int)blockIdx.y == nimg) {   // the extra grid row: the rounding-tie capture of this batch (mcs_tiecap.h), in the same launch
		tie_capture_body(b, nimg, wavesPerImage, maxTies, tieOut, blockIdx.x, gridDim.x);
		return;
	}
	const int img = blockIdx.y, n = d_nkp[img], part = blockIdx.x, parts = gridDim.x;
	auto copy = [&](uint32_t* dst, const uint32_t* src, int rowDw) {   // rows [0, n) of image img: one contiguous run of dwords
		const size_t base = (size_t)img * kpCap * rowDw;
		const int total = n * rowDw;
		for (int i = part * 256 + threadIdx.x; i < total; i += parts * 256) dst[base + i] = src[base + i];
	};
	copy(o.kps, kps, (int)(sizeof(mcs_keypoint) / 4));
	copy(o.desc, desc, descDw);
	copy(o.mask, mask, descDw);
	if (o.rays) copy(o.rays, rays, 6);
	if (part == 0 && threadIdx.x == 0) {
		o.nkp[img] = n;
		if (img == 0) { o.status[0] = *d_status; o.status[1] = *d_ties; }
	}
}
}  // namespace mcs

using namespace mcs;

static bool use_graphs() {   // MCS_GRAPHS=0: every launch of a small batch enqueued one by one (A/B, tests)
	static const bool on = !(getenv("MCS_GRAPHS") && atoi(getenv("MCS_GRAPHS")) == 0);
	return on;
}

// The arguments of one mcs_extract_batch / mcs_extract_batch_strided call (resMask: the masks are the ones mcs_extractor_set_masks left on the device)
struct ExtractCall {
	int nimg; const uint8_t* images; size_t image_pitch; int image_stride; const uint8_t* masks; size_t mask_pitch; int mask_stride; const mcs_ocam* cams; mcs_mem_kind kind;
	int32_t* nkp; mcs_keypoint* keypoints; uint8_t* desc; uint8_t* descmask; double* rays; size_t out_image_pitch_rows; int out_row_stride;
	bool resMask;
};

static int check_inputs(mcs_extractor* e, ExtractCall& a) {
	if (!e || !a.images || !a.nkp || !a.keypoints || !a.desc || !a.descmask) return fail(MCS_ERR_INVALID, "null argument");
	if (a.nimg < 1 || a.nimg > e->maxBatch) return fail(MCS_ERR_INVALID, "nimg exceeds the extractor's max_batch");
	const PyrDesc& hd = e->hd;
	a.resMask = a.masks == MCS_MASKS_RESIDENT;
	if (a.resMask) {
		if (!e->d_resMask || a.nimg > e->resMaskN) return fail(MCS_ERR_INVALID, "MCS_MASKS_RESIDENT: mcs_extractor_set_masks has not been called for this many images");
		a.masks = e->d_resMask; a.mask_pitch = (size_t)hd.width * hd.height; a.mask_stride = hd.width;
	}
	if (a.image_stride < hd.width || (a.masks && a.mask_stride < hd.width)) return fail(MCS_ERR_INVALID, "stride smaller than the image width");
	if (hd.mode != 0 && !a.cams) return fail(MCS_ERR_INVALID, "dBRIEF/mdBRIEF need camera models");
	if (a.rays && !a.cams) return fail(MCS_ERR_INVALID, "rays need camera models");
	return MCS_OK;
}

// everything of `b` that does not depend on where the call's images and outputs lie
static void bind_buffers(const mcs_extractor* e, const ExtractCall& a, ExtractBuffers& b) {
	const PyrDesc& hd = e->hd;
	b.desc = e->d_desc; b.cells = e->d_cells; b.taps = e->d_taps; b.maskMap = e->d_maskMap;
	b.pyr = e->d_pyr; b.blur = e->d_blur; b.slots = e->d_slots; b.cellCount = e->d_cellCount; b.dense = e->d_dense; b.knode = e->d_knode;
	b.denseCount = e->d_denseCount; b.sel = e->d_sel; b.selCount = e->d_selCount; b.selAngle = e->d_selAngle; b.status = e->d_status;
	b.gTab = e->d_gTab; b.aux = e->d_aux; b.fbCount = e->d_fbCount; b.fbList = e->d_fbList; b.preCount = e->d_fbCount + 1; b.preList = e->d_preList;
	b.fbStats = e->d_fbStats; b.tieMin = e->d_tieMin; b.guardEps = e->guardEps; b.describeMode = e->describeMode;
	b.tieCount = e->d_fbCount + 2; b.tieList = e->d_tieList; b.tieTotal = e->d_fbStats + 1;
	b.tieBand = effective_tie_band(e);
	b.sideStream = nullptr; b.evDescFork = nullptr; b.evDescJoin = nullptr;
	b.outImgPitch = a.out_image_pitch_rows ? a.out_image_pitch_rows : (size_t)hd.kpCap;
	b.outRowStride = a.out_row_stride ? a.out_row_stride : hd.descSize;
}

static int check_layout(const mcs_extractor* e, const ExtractCall& a, const ExtractBuffers& b) {
	const PyrDesc& hd = e->hd;
	if (b.outImgPitch < (size_t)hd.kpCap || b.outRowStride < hd.descSize) return fail(MCS_ERR_INVALID, "output image pitch / row stride smaller than the rows they hold");
	// the descriptor kernels store rows as 8-byte words
	if (b.outRowStride % 8 != 0 || (a.kind != MCS_MEM_HOST && (((uintptr_t)a.desc | (uintptr_t)a.descmask) & 7) != 0))
		return fail(MCS_ERR_INVALID, "descriptor / mask rows must be 8-byte aligned (row stride a multiple of 8)");
	if (a.kind != MCS_MEM_HOST && (a.out_image_pitch_rows || a.out_row_stride)) {
		// strided outputs: mask rows either interleaved with the descriptor rows (inside the same stride, behind the descriptor) or a separate array
		const uintptr_t lo = std::min((uintptr_t)a.desc, (uintptr_t)a.descmask), hi = std::max((uintptr_t)a.desc, (uintptr_t)a.descmask);
		const size_t span = ((size_t)(a.nimg - 1) * b.outImgPitch + (size_t)hd.kpCap - 1) * (size_t)b.outRowStride + (size_t)hd.descSize;
		const bool interleaved = hi - lo >= (uintptr_t)hd.descSize && hi - lo + (uintptr_t)hd.descSize <= (uintptr_t)b.outRowStride;
		if (!interleaved && hi - lo < span) return fail(MCS_ERR_INVALID, "descriptor and mask rows overlap for this pitch / stride");
	}
	if (a.kind == MCS_MEM_HOST && (b.outImgPitch != (size_t)hd.kpCap || b.outRowStride != hd.descSize)) return fail(MCS_ERR_UNSUPPORTED, "strided descriptor outputs need device memory");
	{
		// k_blur / k_resize_cols form a lane's level-0 source offset as (image - first image of the wave) * image_pitch in 32 bits; a wave spans 64 / (column groups
		// per image) + 2 images at most
		const unsigned long long ncg = (unsigned long long)((hd.width + 3) / 4), span = 64ull / (ncg ? ncg : 1ull) + 2ull;
		if ((unsigned long long)a.image_pitch * span >= (1ull << 32)) return fail(MCS_ERR_UNSUPPORTED, "image_pitch too large for the level-0 readers (pitch * images per wave must stay below 4 GiB)");
	}
	return MCS_OK;
}

// level 0, masks and outputs of `b`: the caller's device arrays, or (host kind) the extractor's staging, the inputs on their way there
static int stage_inputs(mcs_extractor* e, const ExtractCall& a, ExtractBuffers& b) {
	const PyrDesc& hd = e->hd;
	hipStream_t s = e->ctx->stream;
	if (a.kind == MCS_MEM_HOST) {
		// ONE linear copy per block, in the caller's own layout; the kernels take any pitch / stride for level 0.  (A pitched hipMemcpy2D from pageable
		// host memory is carried out row by row by the runtime: 2 x 480 small transfers per image, ~9 ms per image.)
		const size_t imgSpan = (size_t)(a.nimg - 1) * a.image_pitch + (size_t)(hd.height - 1) * a.image_stride + hd.width;
		HIPCHK(e->inImg.reserve(imgSpan));   // (host-kind calls end with a stream sync, so it is idle here)
		HIPCHK(hipMemcpyAsync(e->inImg.p, a.images, imgSpan, hipMemcpyHostToDevice, s));
		b.img0 = e->inImg.p; b.img0Pitch = a.image_pitch; b.img0Stride = a.image_stride;
		if (a.resMask) { b.mask0 = a.masks; b.mask0Pitch = a.mask_pitch; b.mask0Stride = a.mask_stride; }
		else if (a.masks) {
			const size_t maskSpan = (size_t)(a.nimg - 1) * a.mask_pitch + (size_t)(hd.height - 1) * a.mask_stride + hd.width;
			HIPCHK(e->inMask.reserve(maskSpan));
			HIPCHK(hipMemcpyAsync(e->inMask.p, a.masks, maskSpan, hipMemcpyHostToDevice, s));
			b.mask0 = e->inMask.p; b.mask0Pitch = a.mask_pitch; b.mask0Stride = a.mask_stride;
		}
		b.nkp = e->d_nkp; b.kps = e->d_kps; b.out_desc = e->d_odesc; b.out_mask = e->d_omask; b.rays = a.rays ? e->d_rays : nullptr;
	} else {
		b.img0 = a.images; b.img0Pitch = a.image_pitch; b.img0Stride = a.image_stride;
		b.mask0 = a.masks; b.mask0Pitch = a.mask_pitch; b.mask0Stride = a.mask_stride;
		b.nkp = a.nkp; b.kps = a.keypoints; b.out_desc = a.desc; b.out_mask = a.descmask; b.rays = a.rays;
	}
	return MCS_OK;
}

// The batch's camera models as the kernels read them: each camera's G(s) table from the cache (built on first sight), whether the fast pass serves it, its table's
// index among the batch's distinct ones; the device copies are rewritten only when the batch's models differ from the previous batch's
static int resolve_cameras(mcs_extractor* e, const mcs_ocam* cams, int nimg, ExtractBuffers& b) {
	if (!cams) return MCS_OK;
	const PyrDesc& hd = e->hd;
	hipStream_t s = e->ctx->stream;
	std::vector<OcamDev> hc(nimg);
	std::vector<int> which(nimg), uniq;   // uniq: the cache entries this batch uses, in order of first use (their tables are uploaded once each)
	for (int i = 0; i < nimg; ++i) {
		const mcs_ocam& m = cams[i];
		OcamDev& o = hc[i];
		if (int r = ocam_to_dev(m, &o)) return r;
		// the camera's G(s) table and its bounds: built once per distinct camera
		int w = -1;
		for (size_t k = 0; k < e->camCache.size() && w < 0; ++k) if (memcmp(&e->camCache[k].key, &o, sizeof(o)) == 0) w = (int)k;
		if (w < 0) {
			// (no eviction here: which[] of the earlier images of this batch indexes the cache — it is trimmed after the batch's tables are copied)
			mcs_extractor::CamFast cf;
			cf.key = o; cf.tab.assign(kGTabDoubles, 0.0);
			cf.info = build_g_table(m, cf.tab.data());
			if (!std::isfinite(cf.info.tailU)) cf.tab.assign(kGTabDoubles, 0.0);
			e->camCache.push_back(std::move(cf));
			w = (int)e->camCache.size() - 1;
		}
		which[i] = w;
		const double bound = describe_fast_bound(m, hd.npoints, e->camCache[w].info);
		o.fastOk = bound <= 0.5 * e->guardEps ? 1 : 0;   // a factor 2 between the worst case and the band
		size_t up = std::find(uniq.begin(), uniq.end(), w) - uniq.begin();
		if (up == uniq.size()) uniq.push_back(w);
		o.tabIdx = (int)up;
	}
	if (e->h_cams.size() != hc.size() || memcmp(e->h_cams.data(), hc.data(), sizeof(OcamDev) * hc.size()) != 0) {
		HIPCHK(hipStreamSynchronize(s));   // the previous batch may still read d_cams / d_gTab
		HIPCHK(hipMemcpy(e->d_cams, hc.data(), sizeof(OcamDev) * hc.size(), hipMemcpyHostToDevice));
		std::vector<double> tabs(uniq.size() * (size_t)kGDevDoubles);   // the packed device rows
		for (size_t i = 0; i < uniq.size(); ++i) pack_g_table(e->camCache[uniq[i]].tab.data(), reinterpret_cast<uint8_t*>(&tabs[i * kGDevDoubles]));
		HIPCHK(hipMemcpy(e->d_gTab, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice));
		e->h_cams = hc;
	}
	if (e->camCache.size() > 64) e->camCache.clear();   // a rig has a handful of cameras; a caller that streams distinct models rebuilds (which[] is dead here)
	b.cams = e->d_cams;
	return MCS_OK;
}

// the descriptor stage outside a graph, inside the "describe" bracket of a timing pass
static void enqueue_describe(mcs_ctx* c, const ExtractBuffers& b, const PyrDesc& hd, int nimg) {
	ExtractBuffers bd = b;
	if (c->timing) {   // the dominant kernel alone (k_describe_fast; ORB: k_describe), inside the "describe" bracket
		Timer& t = c->timers["describe_fast"];
		if (!t.a) { (void)hipEventCreate(&t.a); (void)hipEventCreate(&t.b); }
		bd.evFastA = t.a; bd.evFastB = t.b; t.used = true;
	}
	c->tic("describe"); launch_describe(bd, hd, nimg, c->stream); c->toc("describe");
}

// Large batches.  Two chains until the descriptors: the side stream runs the resize chain (7 dependent, latency-bound launches) and then the blur, which needs
// nothing else; the main stream starts FAST on level 0 — the input image itself, a third of all FAST work — at once, picks up the other levels
// when the pyramid is there, and runs the oct-tree.  Both chains leave most of the chip idle on their own.
// (Other launch orders measured in round 3: the whole resize chain first on the main stream, then FAST on all levels in one launch with the blur beside it:
// 2.55 instead of 2.21 ms per step; level 1 first, then FAST on levels 0 and 1 beside the rest of the chain: 2.51.)
static int enqueue_forked(mcs_ctx* c, ExtractBuffers& b, const PyrDesc& hd, int nimg) {
	hipStream_t s = c->stream;
	HIPCHK(hipEventRecord(c->evFork, s));
	HIPCHK(hipStreamWaitEvent(c->side, c->evFork, 0));
	if (hd.chainFits) {
		// the resize chain is one launch (k_resize_chain): FAST on level 0 beside it, then FAST on all other levels in one launch beside the blur
		launch_pyramid(b, hd, nimg, c->side);
		HIPCHK(hipEventRecord(c->evPyr, c->side));
		launch_blur(b, hd, nimg, c->side);
		HIPCHK(hipEventRecord(c->evBlur, c->side));
		launch_fast(b, hd, nimg, s, 0, 1);
		HIPCHK(hipStreamWaitEvent(s, c->evPyr, 0));
		launch_fast(b, hd, nimg, s, 1, hd.nlevels);
	} else {
		// the whole resize chain first, then FAST on all levels in one launch (the blur beside it): the launch orders that start FAST on the first levels earlier lost
		launch_pyramid(b, hd, nimg, c->side, 1, hd.nlevels);
		HIPCHK(hipEventRecord(c->evPyr, c->side));
		launch_blur(b, hd, nimg, c->side);
		HIPCHK(hipEventRecord(c->evBlur, c->side));
		HIPCHK(hipStreamWaitEvent(s, c->evPyr, 0));
		launch_fast(b, hd, nimg, s, 0, hd.nlevels);
	}
	// (holding the previous step's deferred matcher back until here, so that it runs beside the oct-tree / orientation / descriptor kernels instead of
	// beside FAST and the resize chain: measured, 2.22 -> 2.55 ms per step — the descriptor kernel on the critical path suffers more from the company)
	launch_octree(b, hd, nimg, s);   // (oct-trees of levels 0 / 1 on a further stream beside FAST of the rest: measured, no gain)
	HIPCHK(hipStreamWaitEvent(s, c->evBlur, 0));
	b.sideStream = c->side; b.evDescFork = c->evDescFork; b.evDescJoin = c->evDescJoin;   // the side stream is idle again: the main stream has waited for the blur
	enqueue_describe(c, b, hd, nimg);
	return MCS_OK;
}

// the whole launch sequence in order on one stream: what a graph captures, and what runs instead when the capture failed
static void enqueue_in_order(const ExtractBuffers& b, const PyrDesc& hd, int nimg, hipStream_t s) {
	launch_pyramid(b, hd, nimg, s);
	launch_fast(b, hd, nimg, s);
	launch_octree(b, hd, nimg, s);
	launch_blur(b, hd, nimg, s);
	launch_describe(b, hd, nimg, s);
}

// room for one more graph: a caller that rotates output buffers has a few argument sets
static void graph_evict(mcs_extractor* e, hipStream_t s) {
	if (e->graphs.size() >= 4) { (void)hipStreamSynchronize(s); (void)hipGraphExecDestroy(e->graphs.front().exec); e->graphs.erase(e->graphs.begin()); }
}

// The graph of this argument set, captured and cached on first sight; nullptr when the capture failed.
// Capture with an error path: whatever fails between Begin and End, the capture is ENDED (a stream left capturing fails every later call on the context) and
// the graph destroyed; this call and all later ones of the extractor then enqueue their launches one by one (graphs given up: graphMisses forced high).
static hipGraphExec_t graph_find_or_capture(mcs_extractor* e, const ExtractBuffers& b, int nimg, hipStream_t s) {
	// The key is the struct's bytes.  Equal arguments give equal bytes only because extract_impl value-initialises ITS ExtractBuffers (padding zeroed) and every
	// step fills that object in place; `key` and every other copy (e->last, TieSlot::b) are plain copies of it.  A binding step that returned the struct by value
	// or assigned it member-wise from a temporary could leave the padding indeterminate: every call a miss, and replay given up after eight of them.
	for (mcs_extractor::Graph& g : e->graphs)
		if (g.nimg == nimg && memcmp(&g.key, &b, sizeof(b)) == 0) { ++e->graphHits; return g.exec; }
	++e->graphMisses;
	hipGraphExec_t exec = nullptr;
	hipGraph_t graph = nullptr;
	hipError_t ge = hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed);
	if (ge == hipSuccess) {
		enqueue_in_order(b, e->hd, nimg, s);
		const hipError_t le = hipGetLastError();
		ge = hipStreamEndCapture(s, &graph);
		if (ge == hipSuccess && le != hipSuccess) ge = le;
		if (ge == hipSuccess) ge = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
		if (graph) (void)hipGraphDestroy(graph);
	}
	if (ge != hipSuccess) {
		(void)hipGetLastError();
		e->graphMisses = 1000000;   // no further attempts on this extractor
		return nullptr;
	}
	graph_evict(e, s);
	e->graphs.push_back(mcs_extractor::Graph{b, nimg, exec});
	return exec;
}

// Small batches run IN ORDER on the context's stream (round 5): the forks pay for themselves only when the kernels are long — for ONE 3-camera multi-frame the
// kernels take 5-50 us each, and every cross-stream event costs about as much as one of them (extraction of 3 images: 0.33 -> 0.29 ms).
// ONE multi-frame per call is launch-bound: a dozen dependent kernels of 4 - 50 us each, most of them shorter than the host takes to enqueue the next.  The
// sequence is captured once per argument set into a hipGraph and replayed (the copies in and out stay ordinary stream operations around it).
static int enqueue_graph(mcs_extractor* e, const ExtractBuffers& b, int nimg) {
	hipStream_t s = e->ctx->stream;
	hipGraphExec_t exec = graph_find_or_capture(e, b, nimg, s);
	if (!exec) enqueue_in_order(b, e->hd, nimg, s);   // the capture failed: the plain sequence (nothing was enqueued by the failed capture)
	else HIPCHK(hipGraphLaunch(exec, s));
	return MCS_OK;
}

// per-kernel timing passes, MCS_GRAPHS=0, an extractor that has given graphs up: one launch after the other, each stage inside its timer's bracket
static void enqueue_timed(mcs_ctx* c, const ExtractBuffers& b, const PyrDesc& hd, int nimg) {
	hipStream_t s = c->stream;
	c->tic("pyramid"); launch_pyramid(b, hd, nimg, s); c->toc("pyramid");
	c->tic("fast"); launch_fast(b, hd, nimg, s); c->toc("fast");
	c->tic("octree"); launch_octree(b, hd, nimg, s); c->toc("octree");
	c->tic("blur"); launch_blur(b, hd, nimg, s); c->toc("blur");
	enqueue_describe(c, b, hd, nimg);
}

// the end of a host-kind batch: the stream idle, the device status (*st) and the number of listed keypoints (*nties) where the batch's last operations left them
static int finish_host_tail(mcs_extractor* e, hipStream_t s, const int* st, const int* nties, uint8_t* desc, uint8_t* descmask) {
	HIPCHK(hipStreamSynchronize(s));
	if (int r = consume_status(e, *st)) return r;
	// keypoints whose exact arithmetic came within the band of a rounding tie: recomputed here with the host's libm before the results are final
	if (*nties > 0) { if (int r = fix_ties_host(e, *nties, desc, descmask)) return r; }
	return MCS_OK;
}

// host-kind outputs: the staging arrays into the caller's, by one kernel (page-locked outputs) or the runtime's copies
static int finish_host(mcs_extractor* e, const ExtractCall& a, const ExtractBuffers& b) {
	const PyrDesc& hd = e->hd;
	hipStream_t s = e->ctx->stream;
	const size_t rows = (size_t)a.nimg * hd.kpCap;
	int st = 0, nties = 0;
	mcs::ExtractOut o{(int32_t*)device_view(a.nkp), (uint32_t*)device_view(a.keypoints), (uint32_t*)device_view(a.desc), (uint32_t*)device_view(a.descmask),
	                  (uint32_t*)device_view(a.rays), e->h_status ? (int*)device_view(e->h_status) : nullptr};
	static const bool outKernel = !(getenv("MCS_OUT_KERNEL") && atoi(getenv("MCS_OUT_KERNEL")) == 0);   // A/B, tests: 0 = always the runtime's copies
	if (outKernel && o.nkp && o.kps && o.desc && o.mask && o.status && (o.rays || !a.rays)) {
		// page-locked outputs: one launch writes the valid rows (rows past an image's count are left as they are), the counts and the status words
		// (+ one grid row when the extractor has its capture slot: the listed keypoints' windows, usually none)
		hipLaunchKernelGGL(mcs::k_extract_out, dim3(4, a.nimg + (e->hostTie.dev ? 1 : 0)), dim3(256), 0, s, e->d_nkp, (const uint32_t*)e->d_kps, (const uint32_t*)e->d_odesc, (const uint32_t*)e->d_omask,
		                   (const uint32_t*)e->d_rays, e->d_status, e->d_fbCount + 2, o, hd.kpCap, hd.descSize / 4, b, a.nimg, kp_slots_per_image(hd),
		                   kHostTieSlots, e->hostTie.dev);
		HIPCHK(hipGetLastError());
		return finish_host_tail(e, s, &e->h_status[0], &e->h_status[1], a.desc, a.descmask);
	}
	if (e->hostTie.dev) launch_tie_capture(b, hd, a.nimg, kHostTieSlots, e->hostTie.dev, s);
	HIPCHK(hipMemcpyAsync(a.nkp, e->d_nkp, a.nimg * sizeof(int), hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(a.keypoints, e->d_kps, rows * sizeof(mcs_keypoint), hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(a.desc, e->d_odesc, rows * hd.descSize, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(a.descmask, e->d_omask, rows * hd.descSize, hipMemcpyDeviceToHost, s));
	if (a.rays) HIPCHK(hipMemcpyAsync(a.rays, e->d_rays, rows * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(&st, e->d_status, sizeof(int), hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(&nties, e->d_fbCount + 2, sizeof(int), hipMemcpyDeviceToHost, s));
	return finish_host_tail(e, s, &st, &nties, a.desc, a.descmask);
}

static int extract_impl(mcs_extractor* e, ExtractCall a) {
	if (int r = check_inputs(e, a)) return r;
	mcs_ctx* c = e->ctx;
	const PyrDesc& hd = e->hd;
	HIPCHK(hipSetDevice(c->device));

	ExtractBuffers b{};   // value-initialised, then filled in place by the steps below: its bytes are the graph cache's key (graph_find_or_capture)
	bind_buffers(e, a, b);
	if (int r = check_layout(e, a, b)) return r;
	if (int r = stage_inputs(e, a, b)) return r;
	if (int r = resolve_cameras(e, a.cams, a.nimg, b)) return r;

	if (c->overlap() && (long long)a.nimg * hd.width * hd.height >= 4000000ll) { if (int r = enqueue_forked(c, b, hd, a.nimg)) return r; }
	else if (!c->timing && use_graphs() && !(e->graphMisses > 8 && e->graphMisses > e->graphHits)) { if (int r = enqueue_graph(e, b, a.nimg)) return r; }
	else enqueue_timed(c, b, hd, a.nimg);
	HIPCHK(hipGetLastError());
	e->last = b; e->lastN = a.nimg;

	if (a.kind != MCS_MEM_HOST && !e->tieRing.empty()) { if (int r = capture_ties(e, b, a.nimg)) return r; }
	if (a.kind == MCS_MEM_HOST) return finish_host(e, a, b);
	return MCS_OK;
}

extern "C" {

int mcs_extractor_set_masks(mcs_extractor* e, int nimg, const uint8_t* masks, size_t mask_pitch, int mask_stride, mcs_mem_kind kind) {
	if (!e || !masks || nimg < 1 || nimg > e->maxBatch) return fail(MCS_ERR_INVALID, "bad argument");
	const PyrDesc& hd = e->hd;
	if (mask_stride < hd.width) return fail(MCS_ERR_INVALID, "stride smaller than the image width");
	HIPCHK(hipSetDevice(e->ctx->device));
	HIPCHK(hipStreamSynchronize(e->ctx->stream));   // an earlier batch may still read the previous masks
	const size_t plane = (size_t)hd.width * hd.height;
	if (nimg > e->resMaskN) { (void)hipFree(e->d_resMask); e->d_resMask = nullptr; e->resMaskN = 0; HIPCHK(hipMalloc((void**)&e->d_resMask, plane * nimg)); }
	for (int i = 0; i < nimg; ++i)
		HIPCHK(hipMemcpy2D(e->d_resMask + (size_t)i * plane, hd.width, masks + (size_t)i * mask_pitch, mask_stride, hd.width, hd.height,
		                   kind == MCS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
	e->resMaskN = nimg;
	return MCS_OK;
}

int mcs_extract_batch(mcs_extractor* e, int nimg, const uint8_t* images, size_t image_pitch, int image_stride, const uint8_t* masks,
                      size_t mask_pitch, int mask_stride, const mcs_ocam* cams, mcs_mem_kind kind, int32_t* nkp, mcs_keypoint* keypoints,
                      uint8_t* desc, uint8_t* descmask, double* rays) {
	return extract_impl(e, ExtractCall{nimg, images, image_pitch, image_stride, masks, mask_pitch, mask_stride, cams, kind, nkp, keypoints, desc, descmask, rays, 0, 0, false});
}

int mcs_extract_batch_strided(mcs_extractor* e, int nimg, const uint8_t* images, size_t image_pitch, int image_stride, const uint8_t* masks,
                              size_t mask_pitch, int mask_stride, const mcs_ocam* cams, int32_t* nkp, mcs_keypoint* keypoints, uint8_t* desc,
                              uint8_t* descmask, double* rays, size_t out_image_pitch_rows, int out_row_stride) {
	return extract_impl(e, ExtractCall{nimg, images, image_pitch, image_stride, masks, mask_pitch, mask_stride, cams, MCS_MEM_DEVICE, nkp, keypoints, desc, descmask, rays,
	                                   out_image_pitch_rows, out_row_stride, false});
}

int mcs_extractor_status(mcs_extractor* e) {
	if (!e) return fail(MCS_ERR_INVALID, "null");
	int st = 0;
	HIPCHK(hipStreamSynchronize(e->ctx->stream));
	HIPCHK(hipMemcpy(&st, e->d_status, sizeof(int), hipMemcpyDeviceToHost));
	return consume_status(e, st);
}

int mcs_extractor_set_describe(mcs_extractor* e, int exact_only, double guard_eps) {
	if (!e) return fail(MCS_ERR_INVALID, "null");
	if (guard_eps < 0.0 || !(guard_eps < 0.5)) return fail(MCS_ERR_INVALID, "guard band must be in [0, 0.5) pixels (0 = default)");
	HIPCHK(hipStreamSynchronize(e->ctx->stream));
	e->describeMode = exact_only ? 1 : 0;
	e->guardEps = guard_eps > 0.0 ? guard_eps : kDefaultGuardEps;
	e->h_cams.clear();   // fastOk depends on the band: rebuild the device camera table on the next batch
	return MCS_OK;
}

int mcs_extractor_describe_stats(mcs_extractor* e, uint64_t* exact_pass_keypoints, double* guard_eps) {
	if (!e) return fail(MCS_ERR_INVALID, "null");
	HIPCHK(hipStreamSynchronize(e->ctx->stream));
	unsigned long long v = 0;
	HIPCHK(hipMemcpy(&v, e->d_fbStats, sizeof(v), hipMemcpyDeviceToHost));
	if (exact_pass_keypoints) *exact_pass_keypoints = v;
	if (guard_eps) *guard_eps = e->guardEps;
	return MCS_OK;
}

int mcs_selftest_describe_fast(mcs_ctx* c, const mcs_ocam* cam, uint64_t seed, int n, double* max_abs_diff) {
	if (!c || !cam || !max_abs_diff || n < 1) return fail(MCS_ERR_INVALID, "bad argument");
	OcamDev o;
	if (int r = ocam_to_dev(*cam, &o)) return r;
	o.fastOk = 1;
	HIPCHK(hipSetDevice(c->device));
	std::vector<double> tab(kGTabDoubles, 0.0);
	if (!std::isfinite(build_g_table(*cam, tab.data()).tailU)) return fail(MCS_ERR_UNSUPPORTED, "the fast pass does not serve this camera");
	std::vector<double> packed(kGDevDoubles);
	pack_g_table(tab.data(), reinterpret_cast<uint8_t*>(packed.data()));
	unsigned long long got = 0; unsigned long long* dMax = nullptr; const OcamDev* dCam = nullptr; const double* dTab = nullptr;
	Staging st(c, true);
	st.inout(&dMax, &got, sizeof(got)); st.in(&dCam, &o, sizeof(o)); st.in(&dTab, packed.data(), kGDevDoubles * sizeof(double));
	if (int r = st.commit()) return r;
	launch_selftest_fast_model(dCam, dTab, seed, n, cam->width, cam->height, dMax, c->stream);
	HIPCHK(hipGetLastError());
	if (int r = st.finish(MCS_OK)) return r;
	memcpy(max_abs_diff, &got, sizeof(double));
	return MCS_OK;
}

int mcs_extractor_tap_level(mcs_extractor* e, int img, int level, int blurred, uint8_t* out) {
	if (!e || !out || img < 0 || img >= e->lastN || level < 0 || level >= e->hd.nlevels) return fail(MCS_ERR_INVALID, "bad tap");
	HIPCHK(hipStreamSynchronize(e->ctx->stream));
	const LevelInfo& L = e->hd.lv[level];
	const uint8_t* src; int stride;
	if (blurred) { src = e->d_blur + (size_t)img * e->hd.pyrBytes + L.off; stride = L.stride; }
	else src = level_ptr(e->last, e->hd, img, level, &stride);
	HIPCHK(hipMemcpy2D(out, L.w, src, stride, L.w, L.h, hipMemcpyDeviceToHost));
	return MCS_OK;
}

static int tap_list(mcs_extractor* e, int img, int level, const uint32_t* base, const int* counts, int perImage, int lvBase, uint32_t* out,
                    int cap, int* n) {
	HIPCHK(hipStreamSynchronize(e->ctx->stream));
	int cnt = 0;
	HIPCHK(hipMemcpy(&cnt, counts + (size_t)img * e->hd.nlevels + level, sizeof(int), hipMemcpyDeviceToHost));
	*n = cnt;
	const int m = std::min(cnt, cap);
	if (m > 0) HIPCHK(hipMemcpy(out, base + (size_t)img * perImage + lvBase, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return MCS_OK;
}

int mcs_extractor_tap_candidates(mcs_extractor* e, int img, int level, uint32_t* out, int cap, int* n) {
	if (!e || !out || !n || img < 0 || img >= e->lastN || level < 0 || level >= e->hd.nlevels) return fail(MCS_ERR_INVALID, "bad tap");
	return tap_list(e, img, level, e->d_dense, e->d_denseCount, e->hd.densePerImage, e->hd.lv[level].denseBase, out, cap, n);
}

int mcs_extractor_tap_selected(mcs_extractor* e, int img, int level, uint32_t* out, int cap, int* n) {
	if (!e || !out || !n || img < 0 || img >= e->lastN || level < 0 || level >= e->hd.nlevels) return fail(MCS_ERR_INVALID, "bad tap");
	return tap_list(e, img, level, e->d_sel, e->d_selCount, e->hd.selPerImage, e->hd.lv[level].selBase, out, cap, n);
}

}  // extern "C"
