// mcs_host.h — host-side internals shared by the C-ABI translation units (context, error plumbing).
#pragma once
#include "mcs_common.h"
#include "mcs_carve.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

std::string& mcs_err();
inline int fail(int code, const std::string& msg) { mcs_err() = msg; return code; }
#define HIPCHK(expr)                                                                                       \
	do {                                                                                                   \
		hipError_t _e = (expr);                                                                            \
		if (_e != hipSuccess) return fail(MCS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
	} while (0)

static inline int cvRound_(double v) { return (int)lrint(v); }
static inline int cvRoundf_(float v) { return (int)lrintf(v); }
static inline int cvFloor_(double v) { int i = (int)v; return i - (i > v); }
static inline short sat_short(float v) { int iv = cvRoundf_(v); return (short)(iv < -32768 ? -32768 : iv > 32767 ? 32767 : iv); }

struct Timer { hipEvent_t a = nullptr, b = nullptr; bool used = false; };

// the device's view of a page-locked host pointer, or nullptr (pageable memory, another device's allocation): host-kind calls write their outputs straight
// into page-locked arrays with one launch instead of one runtime copy per array (~15 us each for the small arrays of ONE multi-frame)
inline void* device_view(const void* host) {
	if (!host) return nullptr;
	hipPointerAttribute_t a;
	memset(&a, 0, sizeof(a));
	if (hipPointerGetAttributes(&a, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
	if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
	return a.devicePointer;
}

// Grow-only device buffer: at least `bytes` long after reserve(), contents lost when it grows.  Growing goes through hipFree, which waits for the device, so
// nothing still reads the old allocation.  Freed with its owner (context, extractor, keyframe database), whose destroy call has set the device (mcs_ctx_destroy does before `delete c`: keep it that way).
// grow_keep() is the growth that keeps the contents, for a store whose owner sets the capacity schedule itself: exactly `bytes` long afterwards (no slack),
// the first `keep` bytes (<= cap) copied over and the rest zero, both on stream `s` and complete on return.  A failure leaves the buffer as it was.
struct DevBuf {
	uint8_t* p = nullptr; size_t cap = 0;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { if (p) (void)hipFree(p); }
	hipError_t reserve(size_t bytes) {
		if (p && cap >= bytes) return hipSuccess;
		if (p) (void)hipFree(p);
		p = nullptr; cap = 0;
		const size_t want = bytes + bytes / 2 + 256;
		const hipError_t e = hipMalloc((void**)&p, want);
		if (e == hipSuccess) cap = want;
		return e;
	}
	hipError_t grow_keep(size_t bytes, size_t keep, hipStream_t s) {
		if (cap >= bytes) return hipSuccess;
		uint8_t* np = nullptr;
		hipError_t e = hipMalloc((void**)&np, bytes);
		if (e != hipSuccess) return e;
		if (keep) e = hipMemcpyAsync(np, p, keep, hipMemcpyDeviceToDevice, s);
		if (e == hipSuccess) e = hipMemsetAsync(np + keep, 0, bytes - keep, s);
		if (e == hipSuccess) e = hipStreamSynchronize(s);
		if (e != hipSuccess) { (void)hipFree(np); return e; }
		if (p) (void)hipFree(p);
		p = np; cap = bytes;
		return hipSuccess;
	}
	template <class T> T* as() const { return (T*)p; }
};

struct mcs_ctx {
	int device = 0;
	std::vector<mcs_extractor*> extractors;   // live extractors built on this context: mcs_ctx_destroy releases them (their buffers and stream are the context's)
	hipStream_t stream = nullptr;
	bool ownStream = false;
	bool timing = false;
	std::map<std::string, Timer> timers;
	// matcher scratch
	DevBuf partial, partialCount;   // uint32_t / int
	DevBuf topKeys;    // uint32_t: packed [set][K][nq] top-K lists feeding the greedy kernels
	DevBuf topKeys2;   // second list buffer of the deferred searches: the greedy pass of search n reads one while the matcher of search n + 1 fills the other
	DevBuf topCnt;     // int
	DevBuf exA, exW, exRows;   // train sets expanded to matrix-core operands (mcs_match_mfma.hip), per call
	// The ONE block of a call's staged arrays and scratch, and its page-locked mirror (struct Staging below).  No call reads a piece while something else
	// writes it: the pieces of one call are disjoint by construction; a call claims the block (`staging`) before it lays it out and a second claim is an
	// error, so a nested device-kind call (the searches inside mcs_create_new_map_points) cannot carve it again; and the claim is only released behind a
	// synchronisation of the context's stream, so no kernel or copy of an earlier call is still running when the next call overwrites or regrows it.
	DevBuf block;
	uint8_t* mirror = nullptr; size_t mirrorCap = 0;
	bool staging = false;
	// mcs_create_new_map_points: essential matrices, depths, the rotation filter's counter (mcs_newpoints.hip).  A buffer of its own: a device-kind chain
	// returns without a host wait while its kernels (and the greedy pass on the side stream) still use it, so it cannot live in a block that the next
	// call lays out afresh.
	DevBuf npBuf;
	// mcs_frustum / mcs_search_local_points and mcs_search_last_frame / mcs_window_search_frames: per-slot scratch (fresh / active flags, slot cameras, probe
	// windows, candidate lists and counts, the slot matches; mcs_capi_track.hip).  Its own buffer for the same reason: the device-kind call returns while its
	// kernels run, and successive calls reuse it in the order of the context's stream.
	DevBuf lmBuf;
	void* lbaRec = nullptr;   // mcs_local_bundle_adjustment / mcs_optimize_essential_graph: the 64-byte control record the decide kernel leaves in page-locked memory
	// Second HIP stream for the latency-bound / independent kernels (blur next to FAST+oct-tree, the greedy resolution next to the
	// following batch's extraction): they leave most CUs idle, so overlapping them with the VALU-bound kernels is free throughput.
	hipStream_t side = nullptr;    // extraction fork: resize chain + blur beside FAST + oct-tree
	hipStream_t side3 = nullptr;   // deferred searches: the greedy pass, beside the next search's lists on side2
	hipEvent_t evLists = nullptr, evGreedyBuf[2] = {nullptr, nullptr};   // lists of the latest deferred search complete / the greedy pass that read list buffer i complete
	hipStream_t upload = nullptr; unsigned uploadMask = 0; std::vector<hipStream_t> probed; std::vector<unsigned> probedMask;   // mcs_ctx_transfer_stream (mcs_copy.hip)
	hipStream_t side2 = nullptr;   // the greedy match resolution (its own stream: it must not hold up the next batch's resize chain)
	hipEvent_t evFork = nullptr, evPyr = nullptr, evBlur = nullptr, evMatch = nullptr, evGreedy = nullptr;
	hipEvent_t evDescFork = nullptr, evDescJoin = nullptr;   // the exact descriptor pass over the pre-list on `side`, beside the fast pass
	bool greedyPending = false;
	// deferred searches (mcs_ctx_set_async_search): top-K lists AND greedy pass of a device-memory search on side2, completion events in a ring
	bool asyncSearch = false;
	hipEvent_t evSearch[4] = {nullptr, nullptr, nullptr, nullptr};
	long long searchSeq = 0;
	hipStream_t lastResultStream = nullptr;   // the stream the LATEST device-memory search completed its outputs on (search_common records it); nullptr: none yet
	bool overlap() const { return side != nullptr && !timing; }   // per-kernel timing runs everything in order on the main stream

	void tic(const char* name) {
		if (!timing) return;
		Timer& t = timers[name];
		if (!t.a) { (void)hipEventCreate(&t.a); (void)hipEventCreate(&t.b); }
		(void)hipEventRecord(t.a, stream);
	}
	void toc(const char* name) {
		if (!timing) return;
		Timer& t = timers[name];
		(void)hipEventRecord(t.b, stream);
		t.used = true;
	}
	~mcs_ctx() { if (mirror) (void)hipHostFree(mirror); if (lbaRec) (void)hipHostFree(lbaRec); }
};

// make stream `s` wait for the greedy pass that the latest search left on the side stream (its outputs and the buffers it reads are complete behind it)
inline int ctx_join_greedy(mcs_ctx* c, hipStream_t s) {
	if (c->side && c->greedyPending) { HIPCHK(hipStreamWaitEvent(s, c->evGreedy, 0)); c->greedyPending = false; }
	return MCS_OK;
}

inline int bad_polynomial_degree() { return fail(MCS_ERR_INVALID, "bad polynomial degree"); }   // also the rig check of the window family (mcs_window_guard.hip)
// a BowVector CSR as the keyframe database takes it (mcs_kfdb_guard.hip): the offsets first, as a whole, then the words they delimit
int guard_bow_offsets(const int* off, int n, const char* what);
int guard_bow_words(const int* off, int n, const int* w, int nWords, const char* what);
// mcs_ocam -> the kernels' camera model (fastOk / tabIdx stay 0: the extractor sets them)
inline int ocam_to_dev(const mcs_ocam& m, mcs::OcamDev* o) {
	if (m.p_deg < 1 || m.p_deg > MCS_MAX_POLY || m.invP_deg < 1 || m.invP_deg > MCS_MAX_POLY) return bad_polynomial_degree();
	memset(o, 0, sizeof(*o));
	o->c = m.c; o->d = m.d; o->e = m.e; o->u0 = m.u0; o->v0 = m.v0; o->invAffine = m.c - m.d * m.e;
	for (int k = 0; k < m.p_deg; ++k) o->p[k] = m.p[k];
	for (int k = 0; k < m.invP_deg; ++k) o->invP[k] = m.invP[k];
	o->p_deg = m.p_deg; o->invP_deg = m.invP_deg;
	return MCS_OK;
}

// The arrays and the scratch of ONE call, laid out in the context's block.  A piece is declared once (size, pointer to bind, optional host source and
// destination); commit() claims the block, places the pieces (those with a source first, so the copy carries nothing else), binds every pointer and sends
// all sources with ONE H2D copy from the page-locked mirror (a dozen small
// hipMemcpyAsync calls from pageable memory cost ~20 us of runtime overhead each, more than the kernels of a single multi-frame; a hipMalloc / hipFree pair
// per call cost more still); finish() brings the destinations back.  Block and mirror are reused by the next call, so whichever way the call ends after
// commit(), finish() or the destructor synchronises the context's stream before the claim is released.
//   host = false (device-kind call): in() / out() / inout() bind the caller's pointer and declare nothing; only scratch() takes room.  A call without
//   pieces claims nothing and never waits.
//   A piece of zero bytes is legal: it gets an aligned slot of its own (a distinct, valid address) and is never copied.
struct Staging {
	mcs_ctx* c; bool host;
	Carve lay;   // the block's size, known before commit() places the pieces: a slot's size depends on its bytes only, so the sum is the same in any order
	struct Piece { size_t off, bytes; const void* src; void* dst; void** bind; };
	std::vector<Piece> pieces;
	uint8_t* base = nullptr; bool claimed = false;
	Staging(mcs_ctx* ctx, bool hostKind) : c(ctx), host(hostKind) {}
	Staging(const Staging&) = delete;
	Staging& operator=(const Staging&) = delete;
	~Staging() { (void)release(); }

	template <class P> void scratch(P** p, size_t bytes) { add((void**)p, bytes, nullptr, nullptr); }
	template <class P, class T> void upload(P** p, const T* src, size_t bytes) { add((void**)p, bytes, src, nullptr); }   // a host value for either kind
	template <class P, class T> void download(P** p, T* dst, size_t bytes) { add((void**)p, bytes, nullptr, dst); }       // a host result for either kind
	template <class P, class T> void in(P** p, const T* src, size_t bytes) { if (host && src) add((void**)p, bytes, src, nullptr); else *p = (P*)src; }
	template <class P, class T> void out(P** p, T* dst, size_t bytes) { if (host) add((void**)p, bytes, nullptr, dst); else *p = (P*)dst; }   // host, dst null: scratch
	template <class P, class T> void inout(P** p, T* io, size_t bytes) { if (host && io) add((void**)p, bytes, io, io); else *p = (P*)io; }
	size_t bytes() const { return lay.total; }

	// `into`: a device allocation of the caller, bytes() long, instead of the context's block (an object that keeps what it uploads)
	int commit(uint8_t* into = nullptr) {
		if (pieces.empty()) return MCS_OK;
		if (c->staging) return fail(MCS_ERR_UNSUPPORTED, "the context's staging block is in use by the enclosing call");
		if (!into) { HIPCHK(c->block.reserve(lay.total)); into = c->block.p; }
		base = into;
		// the pieces with a source lie first, whatever the order of declaration: the one copy carries nothing else and the mirror covers nothing else
		Carve at;
		size_t hi = 0;
		for (Piece& x : pieces) if (x.src) { x.off = at.take(x.bytes); if (x.bytes) hi = x.off + x.bytes; }
		for (Piece& x : pieces) if (!x.src) x.off = at.take(x.bytes);
		for (const Piece& x : pieces) *x.bind = into + x.off;
		if (c->mirrorCap < hi) {
			if (c->mirror) (void)hipHostFree(c->mirror);
			c->mirror = nullptr; c->mirrorCap = 0;
			HIPCHK(hipHostMalloc((void**)&c->mirror, hi + hi / 2, hipHostMallocDefault));
			c->mirrorCap = hi + hi / 2;
		}
		c->staging = claimed = true;
		for (const Piece& x : pieces)
			if (x.src && x.bytes) memcpy(c->mirror + x.off, x.src, x.bytes);
		if (hi) HIPCHK(hipMemcpyAsync(into, c->mirror, hi, hipMemcpyHostToDevice, c->stream));
		return MCS_OK;
	}
	// rc == MCS_OK: every destination is downloaded (download = false: the caller has brought them back itself); then the stream is synchronised
	int finish(int rc, bool download = true) {
		if (!claimed) return rc;
		hipError_t e = hipSuccess;
		if (rc == MCS_OK && download)
			for (const Piece& x : pieces)
				if (x.dst && x.bytes && e == hipSuccess) e = hipMemcpyAsync(x.dst, base + x.off, x.bytes, hipMemcpyDeviceToHost, c->stream);
		const hipError_t e2 = release();
		if (rc != MCS_OK) return rc;
		if (e != hipSuccess || e2 != hipSuccess) return fail(MCS_ERR_HIP, std::string("staged call: ") + hipGetErrorString(e != hipSuccess ? e : e2));
		return MCS_OK;
	}

private:
	void add(void** bind, size_t bytes, const void* src, void* dst) { lay.take(bytes); pieces.push_back(Piece{0, bytes, src, dst, bind}); }
	hipError_t release() {
		if (!claimed) return hipSuccess;
		const hipError_t e = hipStreamSynchronize(c->stream);
		c->staging = claimed = false;
		return e;
	}
};
