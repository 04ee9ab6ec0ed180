// mcs_extractor.h — the extractor object behind include/mcs_c.h's mcs_extractor*, private to the translation units that build it (mcs_capi.hip), run it
// (mcs_extract.hip) and enforce its rounding ties (mcs_ties.hip); the G(s) table interface of mcs_gtable.hip, which the object caches per camera.
#pragma once
#include "mcs_host.h"

// Guard band of the fast descriptor pass: a coordinate closer than this to a rounding tie sends its keypoint to the exact pass.  2^-24 px: ~4 of
// 10 000 keypoints, and 30-40x above describe_fast_bound() for the Lafida cameras.
static constexpr double kDefaultGuardEps = 5.9604644775390625e-08;
// Default bands around the cvRound ties inside which an exact-arithmetic keypoint is recomputed on the host with the host's libm (mcs_tiefix.hip says why these)
static constexpr double kTieBandOrb = 1e-12, kTieBandDistorted = 1e-9;
static constexpr int kHostTieSlots = 64;   // entries of an extractor's own capture slot (host-kind batches); more listed keypoints take the whole-level download
// recompute_captured (mcs_ties.hip): a pattern sample of a listed keypoint lies outside its 81 x 81 window — a camera whose affine part stretches the pattern beyond
// 40 px (c = 3.2, say: legal input).  Nothing is reported yet: the host-kind caller still has the levels and falls back to them, the pipelined one cannot and fails.
static constexpr int kTieWindowMiss = -1000;

// What build_g_table() (mcs_gtable.hip) knows about one camera's table besides the rows
struct GTabInfo {
	double tailU = INFINITY;   // max over the rows of sqrt(s) * (truncated tail of the row)                       [pixels]
	double rhoB = 0;           // max sqrt(s) * sum_j |g_j| |eps|^j  (>= |rho| on the table's range)
	double dB = 0;             // max sqrt(s) * |s G'(s)|
	double lip = 0;            // max (|G| + 2 |s G'(s)|) >= both eigenvalues of d(x G, y G) / d(x, y)
	double inB = 0;            // max (|G| + 2 |s G'(s)|) * (sqrt(s) + 44): what one relative rounding of the rotated pattern point moves (x G, y G) by — a point
	                           // at distance n from the axis belongs to a keypoint within n + 22 of it, and the rotated offset is within 22: |terms| <= n + 44
	double seen = 0;           // largest |row polynomial - G| (times sqrt(s)) at the sample points checked against direct long double evaluation
	double f32U = INFINITY;    // max sqrt(s) * (what the FLOAT tail of the packed device rows adds: g4, g5, g6 and tau rounded to float, two float FMAs)  [pixels]
};
struct mcs_extractor;

namespace mcs {
GTabInfo build_g_table(const mcs_ocam& m, double* tab);                                   // tab: kGTabDoubles
void pack_g_table(const double* tab, uint8_t* out);                                       // out: kGDevDoubles * 8 bytes
double describe_fast_bound(const mcs_ocam& m, int npoints, const GTabInfo& g);
// mcs_ties.hip, for extract_impl (mcs_extract.hip) and mcs_extractor_destroy
int fix_ties_host(mcs_extractor* e, int nties, uint8_t* h_desc, uint8_t* h_mask);   // host-kind batch, stream idle: the listed keypoints recomputed into the host rows
int capture_ties(mcs_extractor* e, const ExtractBuffers& b, int nimg);              // device-kind batch: its listed keypoints into the next ring slot, behind the descriptor kernels
void free_tie_capture(mcs_extractor* e);
extern const signed char kPattern[2048];   // the learned pattern (mcs_capi.hip)
void describe_host(int mode, int descSize, const signed char* pattern, const OcamDev* cam, int undistort, int level, float levelScale, int row, int col, float angle,
                   const HostLevel& L, uint8_t* desc, uint8_t* mask);   // mcs_tiefix.hip
void launch_tie_capture(const ExtractBuffers& b, const PyrDesc& hd, int nimg, int maxTies, uint8_t* devOut, hipStream_t s);   // mcs_tiefix.hip
}  // namespace mcs

struct mcs_extractor {
	mcs_ctx* ctx = nullptr;
	mcs_extractor_params params{};
	int maxBatch = 0;
	mcs::PyrDesc hd{};
	std::vector<mcs::CellInfo> cells;
	mcs::PyrDesc* d_desc = nullptr;
	mcs::CellInfo* d_cells = nullptr;
	mcs::ResizeTap* d_taps = nullptr;
	short* d_maskMap = nullptr;
	uint8_t *d_pyr = nullptr, *d_blur = nullptr;
	uint32_t *d_slots = nullptr, *d_dense = nullptr, *d_sel = nullptr;
	float* d_selAngle = nullptr;
	unsigned short* d_knode = nullptr;
	int *d_cellCount = nullptr, *d_denseCount = nullptr, *d_selCount = nullptr, *d_status = nullptr;
	mcs::OcamDev* d_cams = nullptr;
	std::vector<mcs::OcamDev> h_cams;
	// descriptor passes (mcs_describe.hip): fallback list of the fast pass, its running total, the guard band
	int* d_fbCount = nullptr; uint32_t *d_fbList = nullptr, *d_preList = nullptr; unsigned long long* d_fbStats = nullptr; unsigned long long* d_tieMin = nullptr; void* d_aux = nullptr;   // d_fbCount: [0] fallback list, [1] pre-list
	int describeMode = 0; double guardEps = kDefaultGuardEps;
	// rounding ties of the exact arithmetic (mcs_tiefix.hip): the batch's listed keypoints, the band (0 = the mode's default, < 0 = list nothing), totals
	uint32_t* d_tieList = nullptr; double tieBand = 0.0; unsigned long long tieFixed = 0;
	// pipelined enforcement (mcs_extractor_set_tie_capture): a ring of page-locked capture slots, one per device-kind batch in flight
	struct TieSlot { uint8_t* host = nullptr; uint8_t* dev = nullptr; hipEvent_t ev = nullptr; mcs::ExtractBuffers b{}; int nimg = 0; std::vector<mcs::OcamDev> cams; long long seq = -1; bool patched = false; };
	std::vector<TieSlot> tieRing; int tieMax = 0; long long batchSeq = 0; hipStream_t patchStream = nullptr; uint8_t* h_patchRows = nullptr;
	unsigned long long tieWindowMisses = 0;
	TieSlot hostTie;   // host-kind batches: the extractor's own capture slot (kHostTieSlots entries)
	// G(s) tables of the cameras seen so far (a rig has a handful), and the batch's distinct tables as the fast pass reads them
	struct CamFast { mcs::OcamDev key; GTabInfo info; std::vector<double> tab; };
	std::vector<CamFast> camCache;
	double* d_gTab = nullptr;
	// host-kind input staging: the caller's image / mask block as it lies in host memory (same pitch and stride), grown on demand
	DevBuf inImg, inMask;
	// host-kind output staging
	int* d_nkp = nullptr; mcs_keypoint* d_kps = nullptr; uint8_t *d_odesc = nullptr, *d_omask = nullptr; double* d_rays = nullptr;
	mcs::ExtractBuffers last{};
	int lastN = 0;
	// mirror masks kept on the device (mcs_extractor_set_masks): tight rows, one after the other
	uint8_t* d_resMask = nullptr; int resMaskN = 0;
	int* h_status = nullptr;   // page-locked: device status + tie count of a host-kind batch, written by k_extract_out
	// hipGraphs of the in-order launch sequence (small batches, extract_impl): keyed by the kernels' arguments
	struct Graph { mcs::ExtractBuffers key; int nimg; hipGraphExec_t exec; };
	std::vector<Graph> graphs;
	long graphHits = 0, graphMisses = 0;   // a caller that rotates through more argument sets than the cache holds would re-capture on every call: replay is given up then
};

// the band the kernels list ties in: the caller's, nothing (< 0), or the mode's default
inline double effective_tie_band(const mcs_extractor* e) {
	return e->tieBand > 0.0 ? e->tieBand : (e->tieBand < 0.0 ? -1.0 : (e->hd.mode == 0 ? kTieBandOrb : kTieBandDistorted));
}

// the device status word as the caller has read it (`st`; the stream is idle): non-zero is cleared on the device and reported
inline int consume_status(mcs_extractor* e, int st) {
	if (st == 0) return MCS_OK;
	(void)hipMemset(e->d_status, 0, sizeof(int));
	return fail(st, "device capacity exceeded during extraction");
}

