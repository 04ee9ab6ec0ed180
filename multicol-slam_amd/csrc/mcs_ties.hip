// mcs_ties.hip — enforcement of the exact arithmetic's rounding ties on the host side of the C ABI (mcs_tiefix.hip says why and holds describe_host and the
// capture kernel): the whole-level download (fix_ties), the captured windows of host-kind batches (fix_ties_host) and of pipelined device-kind batches (the ring:
// mcs_extractor_set_tie_capture / capture_ties / mcs_extractor_patch_ties), the band and the counters.
#include "mcs_extractor.h"

using namespace mcs;

// The listed keypoints of the extractor's LAST batch (ExtractBuffers.tieList) through describe_host; the stream must be idle.  The recomputed rows replace the
// device outputs in place and, when given, the host copies (tight [image][kpCap][descSize] arrays).
static int fix_ties(mcs_extractor* e, int nties, uint8_t* h_desc, uint8_t* h_mask) {
	const PyrDesc& hd = e->hd;
	const ExtractBuffers& b = e->last;
	const int wavesPerImage = kp_slots_per_image(hd);
	const int cap = e->maxBatch * wavesPerImage;
	if (nties > cap) nties = cap;
	std::vector<uint32_t> list(nties);
	HIPCHK(hipMemcpy(list.data(), e->d_tieList, sizeof(uint32_t) * nties, hipMemcpyDeviceToHost));
	std::sort(list.begin(), list.end());   // by image, then slot: one download per (image, level)
	struct Lv { std::vector<uint8_t> blur, raw; };
	std::map<std::pair<int, int>, Lv> levels;
	std::vector<int> selCount(hd.nlevels);
	int curImg = -1;
	std::vector<uint8_t> dsc(hd.descSize), msk(hd.descSize);
	for (uint32_t gw : list) {
		const int img = (int)(gw / (uint32_t)wavesPerImage), sl = (int)(gw - (uint32_t)img * wavesPerImage);
		if (img >= e->lastN || sl >= hd.kpCap) continue;
		if (img != curImg) { HIPCHK(hipMemcpy(selCount.data(), e->d_selCount + (size_t)img * hd.nlevels, sizeof(int) * hd.nlevels, hipMemcpyDeviceToHost)); curImg = img; levels.clear(); }
		int level = -1, pos = 0, total = 0;
		for (int l = 0; l < hd.nlevels; ++l) { if (sl >= total && sl < total + selCount[l]) { level = l; pos = sl - total; } total += selCount[l]; }
		if (level < 0) continue;
		const LevelInfo& L = hd.lv[level];
		uint32_t rec = 0; float angle = 0.f;
		HIPCHK(hipMemcpy(&rec, e->d_sel + (size_t)img * hd.selPerImage + L.selBase + pos, sizeof(rec), hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(&angle, e->d_selAngle + (size_t)img * hd.selPerImage + L.selBase + pos, sizeof(angle), hipMemcpyDeviceToHost));
		Lv& lv = levels[std::make_pair(img, level)];
		if (lv.blur.empty()) {
			lv.blur.resize((size_t)L.w * L.h); lv.raw.resize((size_t)L.w * L.h);
			int rstride = 0;
			const uint8_t* raw = level_ptr(b, hd, img, level, &rstride);
			HIPCHK(hipMemcpy2D(lv.blur.data(), L.w, e->d_blur + (size_t)img * hd.pyrBytes + L.off, L.stride, L.w, L.h, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy2D(lv.raw.data(), L.w, raw, rstride, L.w, L.h, hipMemcpyDeviceToHost));
		}
		HostLevel hl{lv.blur.data(), lv.raw.data(), L.w, L.h};
		const int col = (int)(rec & 0xFFF) + kMinBorder, row = (int)((rec >> 12) & 0xFFF) + kMinBorder;
		const OcamDev* cam = hd.mode != 0 && (size_t)img < e->h_cams.size() ? &e->h_cams[img] : nullptr;
		if (hd.mode != 0 && !cam) return fail(MCS_ERR_INVALID, "internal: tie list without camera models");
		describe_host(hd.mode, hd.descSize, kPattern, cam, hd.undistort, level, L.scale, row, col, angle, hl, dsc.data(), msk.data());
		const size_t drow = ((size_t)img * b.outImgPitch + sl) * b.outRowStride;
		HIPCHK(hipMemcpy(b.out_desc + drow, dsc.data(), hd.descSize, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(b.out_mask + drow, msk.data(), hd.descSize, hipMemcpyHostToDevice));
		if (h_desc) memcpy(h_desc + ((size_t)img * hd.kpCap + sl) * hd.descSize, dsc.data(), hd.descSize);
		if (h_mask) memcpy(h_mask + ((size_t)img * hd.kpCap + sl) * hd.descSize, msk.data(), hd.descSize);
		e->tieFixed++;
	}
	const int zero = 0;
	HIPCHK(hipMemcpy(e->d_fbCount + 2, &zero, sizeof(int), hipMemcpyHostToDevice));   // done: a second call finds nothing
	return MCS_OK;
}

// The listed keypoints of a batch from what k_tie_capture left in page-locked memory (mcs_tiefix.hip): entry i -> descriptor | mask rows at rowsOut + i * 2 *
// descSize, its image and slot in where[i]; returns the number of rows recomputed, kTieWindowMiss (mcs_extractor.h), or < 0 = error code.  No device access at all.
static int recompute_captured(mcs_extractor* e, const uint8_t* slot, int n, const std::vector<OcamDev>& cams, uint8_t* rowsOut, std::vector<std::pair<int, int> >& where) {
	const PyrDesc& hd = e->hd;
	const int wavesPerImage = kp_slots_per_image(hd);
	where.clear();
	for (int i = 0; i < n; ++i) {
		const TieCaptureEntry* en = reinterpret_cast<const TieCaptureEntry*>(slot + sizeof(TieCaptureHeader) + (size_t)i * sizeof(TieCaptureEntry));
		if (en->level < 0 || en->level >= hd.nlevels) continue;
		const int img = (int)(en->gw / (uint32_t)wavesPerImage), sl = (int)(en->gw - (uint32_t)img * wavesPerImage);
		const LevelInfo& L = hd.lv[en->level];
		const int col = (int)(en->rec & 0xFFF) + kMinBorder, row = (int)((en->rec >> 12) & 0xFFF) + kMinBorder;
		const OcamDev* cam = hd.mode != 0 && (size_t)img < cams.size() ? &cams[img] : nullptr;
		if (hd.mode != 0 && !cam) return fail(MCS_ERR_INVALID, "internal: tie capture without camera models");
		bool miss = false;
		HostLevel hl{nullptr, nullptr, L.w, L.h, en->patch, row - kTiePatchR, col - kTiePatchR, kTiePatchDim, &miss};
		uint8_t* dsc = rowsOut + where.size() * 2 * hd.descSize;
		describe_host(hd.mode, hd.descSize, kPattern, cam, hd.undistort, en->level, L.scale, row, col, en->angle, hl, dsc, dsc + hd.descSize);
		if (miss) { ++e->tieWindowMisses; return kTieWindowMiss; }
		where.push_back(std::make_pair(img, sl));
	}
	return (int)where.size();
}

// Host-kind batches: the listed keypoints from the extractor's own capture slot (written by k_tie_capture in front of the batch's final synchronisation) — a few
// microseconds per keypoint, no device access; the whole-level download of fix_ties only when more keypoints are listed than the slot holds (widened bands) or
// when a sample misses a captured window (a camera that stretches the pattern beyond 40 px)
int mcs::fix_ties_host(mcs_extractor* e, int nties, uint8_t* h_desc, uint8_t* h_mask) {
	const PyrDesc& hd = e->hd;
	if (!e->hostTie.host || nties > kHostTieSlots) return fix_ties(e, nties, h_desc, h_mask);
	std::vector<std::pair<int, int> > where;
	std::vector<uint8_t> rows((size_t)nties * 2 * hd.descSize);
	const int done = recompute_captured(e, e->hostTie.host, nties, e->h_cams, rows.data(), where);
	if (done == kTieWindowMiss) return fix_ties(e, nties, h_desc, h_mask);   // this batch's levels are still resident: every listed keypoint from them instead
	if (done < 0) return done;
	for (int i = 0; i < done; ++i) {
		const size_t r = ((size_t)where[i].first * hd.kpCap + where[i].second) * hd.descSize;
		if (h_desc) memcpy(h_desc + r, rows.data() + (size_t)i * 2 * hd.descSize, hd.descSize);
		if (h_mask) memcpy(h_mask + r, rows.data() + (size_t)i * 2 * hd.descSize + hd.descSize, hd.descSize);
	}
	e->tieFixed += (unsigned long long)done;
	return MCS_OK;
}

// pipelined enforcement: what the host needs of this batch's listed keypoints leaves for page-locked memory right behind the descriptor kernels; the
// caller patches the rows one step later (mcs_extractor_patch_ties), while the pyramid buffers already hold the next batch
int mcs::capture_ties(mcs_extractor* e, const ExtractBuffers& b, int nimg) {
	const PyrDesc& hd = e->hd;
	hipStream_t s = e->ctx->stream;
	mcs_extractor::TieSlot& t = e->tieRing[(size_t)(e->batchSeq % (long long)e->tieRing.size())];
	launch_tie_capture(b, hd, nimg, e->tieMax, t.dev, s);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(t.ev, s));
	t.b = b; t.nimg = nimg; t.seq = e->batchSeq; t.patched = false;
	if (hd.mode != 0) t.cams = e->h_cams; else t.cams.clear();
	++e->batchSeq;
	return MCS_OK;
}

void mcs::free_tie_capture(mcs_extractor* e) {
	for (mcs_extractor::TieSlot& t : e->tieRing) { if (t.ev) (void)hipEventDestroy(t.ev); if (t.host) (void)hipHostFree(t.host); }
	e->tieRing.clear(); e->tieMax = 0;
	if (e->h_patchRows) { (void)hipHostFree(e->h_patchRows); e->h_patchRows = nullptr; }
	if (e->patchStream) { (void)hipStreamSynchronize(e->patchStream); (void)hipStreamDestroy(e->patchStream); e->patchStream = nullptr; }
}

extern "C" {

int mcs_extractor_tie_stats(mcs_extractor* e, double* min_tie_distance, int reset) {
	if (!e) return fail(MCS_ERR_INVALID, "null");
	HIPCHK(hipStreamSynchronize(e->ctx->stream));
	unsigned long long v = 0;
	HIPCHK(hipMemcpy(&v, e->d_tieMin, sizeof(v), hipMemcpyDeviceToHost));
	if (min_tie_distance) memcpy(min_tie_distance, &v, sizeof(double));
	if (reset) { const unsigned long long inf = 0x7FF0000000000000ull; HIPCHK(hipMemcpy(e->d_tieMin, &inf, sizeof(inf), hipMemcpyHostToDevice)); }
	return MCS_OK;
}

int mcs_extractor_set_tie_band(mcs_extractor* e, double band_px) {
	if (!e) return fail(MCS_ERR_INVALID, "null");
	if (!(band_px <= 0.5)) return fail(MCS_ERR_INVALID, "tie band must be <= 0.5 pixels (0 = default, < 0 = list nothing)");
	HIPCHK(hipStreamSynchronize(e->ctx->stream));
	e->tieBand = band_px;
	return MCS_OK;
}

int mcs_extractor_fix_ties(mcs_extractor* e, int* recomputed) {
	if (!e) return fail(MCS_ERR_INVALID, "null");
	if (recomputed) *recomputed = 0;
	if (e->lastN <= 0) return MCS_OK;
	HIPCHK(hipSetDevice(e->ctx->device));
	HIPCHK(hipStreamSynchronize(e->ctx->stream));
	int nties = 0;
	HIPCHK(hipMemcpy(&nties, e->d_fbCount + 2, sizeof(int), hipMemcpyDeviceToHost));
	if (nties <= 0) return MCS_OK;
	const unsigned long long before = e->tieFixed;
	if (int r = fix_ties(e, nties, nullptr, nullptr)) return r;
	if (recomputed) *recomputed = (int)(e->tieFixed - before);
	return MCS_OK;
}

int mcs_extractor_set_tie_capture(mcs_extractor* e, int depth, int max_ties) {
	if (!e || depth < 0 || depth > 16 || max_ties < 0 || max_ties > 4096) return fail(MCS_ERR_INVALID, "depth must be 0..16, max_ties 0..4096 (0 = default 64)");
	HIPCHK(hipSetDevice(e->ctx->device));
	HIPCHK(hipStreamSynchronize(e->ctx->stream));
	free_tie_capture(e);
	if (depth == 0) return MCS_OK;
	if (max_ties == 0) max_ties = 64;
	const size_t bytes = sizeof(TieCaptureHeader) + (size_t)max_ties * sizeof(TieCaptureEntry);
	e->tieRing.resize(depth);
	for (mcs_extractor::TieSlot& t : e->tieRing) {
		if (hipHostMalloc((void**)&t.host, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); free_tie_capture(e); return fail(MCS_ERR_HIP, "page-locked capture slot"); }
		memset(t.host, 0, sizeof(TieCaptureHeader));
		t.dev = (uint8_t*)device_view(t.host);
		if (!t.dev || hipEventCreateWithFlags(&t.ev, hipEventDisableTiming | hipEventReleaseToSystem) != hipSuccess) { (void)hipGetLastError(); free_tie_capture(e); return fail(MCS_ERR_HIP, "capture slot: device view / event"); }
	}
	if (hipHostMalloc((void**)&e->h_patchRows, (size_t)max_ties * 2 * e->hd.descSize, hipHostMallocDefault) != hipSuccess ||
	    hipStreamCreateWithFlags(&e->patchStream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); free_tie_capture(e); return fail(MCS_ERR_HIP, "patch stream / staging rows"); }
	e->tieMax = max_ties;
	return MCS_OK;
}

int mcs_extractor_patch_ties(mcs_extractor* e, int back, int* listed, int* recomputed) {
	if (listed) *listed = 0;
	if (recomputed) *recomputed = 0;
	if (!e || back < 0) return fail(MCS_ERR_INVALID, "bad argument");
	if (e->tieRing.empty()) return fail(MCS_ERR_INVALID, "mcs_extractor_set_tie_capture has not been called");
	const long long seq = e->batchSeq - 1 - back;
	if (seq < 0) return MCS_OK;   // no such batch yet (the first steps of a pipeline)
	mcs_extractor::TieSlot& t = e->tieRing[(size_t)(seq % (long long)e->tieRing.size())];
	if (t.seq != seq) return fail(MCS_ERR_INVALID, "that batch's capture slot has been reused (capture depth too small for this lag)");
	HIPCHK(hipSetDevice(e->ctx->device));
	HIPCHK(hipEventSynchronize(t.ev));
	const TieCaptureHeader* hdr = reinterpret_cast<const TieCaptureHeader*>(t.host);
	const int n = hdr->count;
	if (listed) *listed = n;
	if (n <= 0 || t.patched) return MCS_OK;
	if (n > e->tieMax) return fail(MCS_ERR_CAPACITY, "more keypoints inside the tie band than the capture slots hold (mcs_extractor_set_tie_capture max_ties); use mcs_extractor_fix_ties for this band");
	const PyrDesc& hd = e->hd;
	const ExtractBuffers& b = t.b;
	std::vector<std::pair<int, int> > where;
	const int done = recompute_captured(e, t.host, n, t.cams, e->h_patchRows, where);
	// (no way back here: the pyramid buffers may hold a later batch already.  Nothing is patched, the slot stays unpatched)
	if (done == kTieWindowMiss) return fail(MCS_ERR_UNSUPPORTED, "a pattern sample of a listed keypoint lies outside the captured 81 x 81 window (camera model with > 1.9x local magnification): use host-kind batches or mcs_extractor_fix_ties with this camera");
	if (done < 0) return done;
	for (int i = 0; i < done; ++i) {
		const uint8_t* dsc = e->h_patchRows + (size_t)i * 2 * hd.descSize;
		const size_t drow = ((size_t)where[i].first * b.outImgPitch + where[i].second) * b.outRowStride;
		HIPCHK(hipMemcpyAsync(b.out_desc + drow, dsc, hd.descSize, hipMemcpyHostToDevice, e->patchStream));
		HIPCHK(hipMemcpyAsync(b.out_mask + drow, dsc + hd.descSize, hd.descSize, hipMemcpyHostToDevice, e->patchStream));
	}
	// the rows are in place before this returns: whatever the caller enqueues next (matcher, exchange, download) reads the host's arithmetic
	HIPCHK(hipStreamSynchronize(e->patchStream));
	e->tieFixed += (unsigned long long)done;
	t.patched = true;
	if (recomputed) *recomputed = done;
	return MCS_OK;
}

int mcs_extractor_tie_counts(mcs_extractor* e, uint64_t* listed, uint64_t* recomputed, double* band_px) {
	if (!e) return fail(MCS_ERR_INVALID, "null");
	HIPCHK(hipStreamSynchronize(e->ctx->stream));
	unsigned long long v = 0;
	HIPCHK(hipMemcpy(&v, e->d_fbStats + 1, sizeof(v), hipMemcpyDeviceToHost));
	if (listed) *listed = v;
	if (recomputed) *recomputed = e->tieFixed;
	if (band_px) *band_px = effective_tie_band(e);
	return MCS_OK;
}

}  // extern "C"
