// mcs_bow.hip — cMultiFrame::ComputeBoW (src/cMultiFrame.cpp:356-363): the DBoW2 vocabulary-tree descent of every descriptor
// (ThirdParty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1259 with FORB::distance, FORB.cpp:85-105), SURVEY §8f row 4.
// One lane per feature: the descriptor (32 bytes, what FORB compares) sits in 8 VGPRs, every level reads the <= k child descriptors of the
// current node (the small vocabulary — 8823 nodes x 32 B — stays in L2) and keeps the first strict minimum, like the reference.
// Outputs per feature: the leaf node reached and the node of the path at level L - levelsup; word ids, weights and the BowVector /
// FeatureVector maps are table look-ups and a sort on the host; mcs_bow_vector builds the BowVector of one multi-frame from the leaf nodes on the device
// (TemplatedVocabulary.h:1127-1205, BowVector.cpp normalize), from the word table of mcs_vocabulary_set_words (m_nodes[i].word_id / weight).
#include "mcs_host.h"

namespace mcs {

struct BowArgs {
	const uint8_t* nodeDesc; const int* childOff; const int* childIdx; int L;
	const uint8_t* desc; int n; int stride; int levelsup;
	int* leaf; int* nid;
};

__global__ __launch_bounds__(256) void k_bow_transform(BowArgs a) {
	const int f = blockIdx.x * 256 + threadIdx.x;
	if (f >= a.n) return;
	uint32_t q[8];
	const uint32_t* qp = reinterpret_cast<const uint32_t*>(a.desc + (size_t)f * a.stride);
#pragma unroll
	for (int w = 0; w < 8; ++w) q[w] = qp[w];
	const int nidLevel = a.L - a.levelsup;
	int nidv = 0, cur = 0, level = 0;
	for (int guard = 0; guard < 64; ++guard) {
		++level;
		const int lo = a.childOff[cur], hi = a.childOff[cur + 1];
		int best = 0x7FFFFFFF, bestId = cur;
		for (int c = lo; c < hi; ++c) {
			const int id = a.childIdx[c];
			const uint4* np = reinterpret_cast<const uint4*>(a.nodeDesc + 32 * (size_t)id);
			const uint4 n0 = np[0], n1 = np[1];
			const int d = __popc(q[0] ^ n0.x) + __popc(q[1] ^ n0.y) + __popc(q[2] ^ n0.z) + __popc(q[3] ^ n0.w) + __popc(q[4] ^ n1.x) +
			              __popc(q[5] ^ n1.y) + __popc(q[6] ^ n1.z) + __popc(q[7] ^ n1.w);
			if (d < best) { best = d; bestId = id; }   // the first child starts the minimum, later ones need strictly less
		}
		cur = bestId;
		if (level == nidLevel) nidv = cur;
		if (a.childOff[cur + 1] - a.childOff[cur] <= 0) break;   // isLeaf()
	}
	a.leaf[f] = cur;
	a.nid[f] = nidv;
}

// BowVector of one frame from its leaf nodes (TemplatedVocabulary::transform, TF_IDF branch :1147-1163, then BowVector::normalize(L1)).
// Every addend of a word is that word's one weight, so the value is `count` sequential additions of it; no sort of the features is needed.
// hist (n_words ints) is zero between calls: the kernel clears what it touched.
__global__ __launch_bounds__(1024) void k_bow_vector(const int* leaf, int n, int nNodes, int nWords, const int* wordOf, const double* weightOf, int* hist, int* dW,
                                                     double* dWt, int* outW, double* outV, int* nOut, int* err) {
	__shared__ int sd;
	__shared__ double snorm;
	if (threadIdx.x == 0) sd = 0;
	__syncthreads();
	for (int i = threadIdx.x; i < n; i += 1024) {
		const int nd = leaf[i];
		if (nd < 0 || nd >= nNodes) { atomicOr(err, 1); continue; }
		const double w = weightOf[nd];
		if (!(w > 0)) continue;
		const int wid = wordOf[nd];
		if (wid < 0 || wid >= nWords) { atomicOr(err, 2); continue; }
		if (atomicAdd(&hist[wid], 1) == 0) {
			const int k = atomicAdd(&sd, 1);
			dW[k] = wid; dWt[k] = w;
		}
	}
	__syncthreads();
	const int d = sd;
	for (int k = threadIdx.x; k < d; k += 1024) {
		const int wid = dW[k];
		int r = 0;
		for (int j = 0; j < d; ++j) r += dW[j] < wid;
		const double w = dWt[k];
		double v = w;
		for (int c = hist[wid]; c > 1; --c) v += w;
		outW[r] = wid;
		outV[r] = v;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		double norm = 0.0;
		for (int r = 0; r < d; ++r) norm += fabs(outV[r]);
		snorm = norm;
		*nOut = d;
	}
	__syncthreads();
	const double norm = snorm;
	for (int k = threadIdx.x; k < d; k += 1024) {
		if (norm > 0.0) outV[k] /= norm;
		hist[dW[k]] = 0;
	}
}

}  // namespace mcs

using namespace mcs;

// Both halves are one buffer each, laid out and filled by the Staging that uploads them (as mcs_sim3_create keeps what it uploads).
struct mcs_vocabulary {
	mcs_ctx* ctx = nullptr;
	int nNodes = 0, L = 0;
	DevBuf tree;
	const uint8_t* nodeDesc = nullptr; const int* childOff = nullptr; const int* childIdx = nullptr;
	// word id and weight of every node (mcs_vocabulary_set_words) and a zeroed per-word histogram for mcs_bow_vector; wordOf is null until a table is set
	DevBuf table;
	int nWords = 0; const int* wordOf = nullptr; const double* weightOf = nullptr; int* hist = nullptr;
};

int mcs_vocabulary_set_words(mcs_vocabulary* v, const int32_t* word_id_per_node, const double* weight_per_node) {
	if (!v || !word_id_per_node || !weight_per_node) return fail(MCS_ERR_INVALID, "null argument");
	int mx = -1;
	for (int i = 0; i < v->nNodes; ++i) {
		if (word_id_per_node[i] < -1) return fail(MCS_ERR_INVALID, "word ids must be >= 0 (-1: an inner node)");
		if (!(weight_per_node[i] >= 0.0) || std::isinf(weight_per_node[i])) return fail(MCS_ERR_INVALID, "weights must be finite and >= 0 (TF-IDF)");
		mx = std::max(mx, (int)word_id_per_node[i]);
	}
	// DBoW2 gives every leaf a word id of its own.  k_bow_vector takes a word's ONE weight from whichever node reaches the histogram bin first, so two weighted
	// nodes of one word would make the value a race.  Nodes of weight 0 never reach the histogram and may share an id.
	std::vector<int> weighted;
	for (int i = 0; i < v->nNodes; ++i)
		if (weight_per_node[i] > 0.0 && word_id_per_node[i] >= 0) weighted.push_back(word_id_per_node[i]);
	std::sort(weighted.begin(), weighted.end());
	if (std::adjacent_find(weighted.begin(), weighted.end()) != weighted.end())
		return fail(MCS_ERR_INVALID, "two nodes with a weight > 0 carry the same word id (every word has one leaf)");
	mcs_ctx* c = v->ctx;
	HIPCHK(hipSetDevice(c->device));
	const size_t nn = (size_t)v->nNodes, nw = (size_t)std::max(mx + 1, 1);
	v->wordOf = nullptr; v->nWords = 0;   // from here on the stored table is being replaced: there is none until the new one is complete
	Staging stg(c, true);
	stg.upload(&v->wordOf, word_id_per_node, nn * 4); stg.upload(&v->weightOf, weight_per_node, nn * 8); stg.scratch(&v->hist, nw * 4);
	hipError_t e = v->table.reserve(stg.bytes());
	if (e == hipSuccess && stg.commit(v->table.p) != MCS_OK) e = hipErrorUnknown;
	if (e == hipSuccess) e = hipMemsetAsync(v->hist, 0, nw * 4, c->stream);
	if (stg.finish(e == hipSuccess ? MCS_OK : MCS_ERR_HIP) != MCS_OK) { v->wordOf = nullptr; return fail(MCS_ERR_HIP, "vocabulary word upload failed"); }
	v->nWords = (int)nw;
	return MCS_OK;
}

int mcs_vocabulary_create(mcs_ctx* c, int n_nodes, const uint8_t* node_desc, const int32_t* child_off, const int32_t* child_idx, int L,
                          mcs_vocabulary** out) {
	if (!c || !node_desc || !child_off || !child_idx || !out) return fail(MCS_ERR_INVALID, "null argument");
	if (n_nodes < 2 || L < 1) return fail(MCS_ERR_INVALID, "a vocabulary needs a root, at least one child and L >= 1");
	// validate the tree: offsets monotone, children in range, the root has children, no self loops (the descent must terminate)
	if (child_off[0] != 0 || child_off[1] <= 0) return fail(MCS_ERR_INVALID, "the root (node 0) must have children");
	for (int i = 0; i < n_nodes; ++i) {
		if (child_off[i + 1] < child_off[i]) return fail(MCS_ERR_INVALID, "child_off must be non-decreasing");
		for (int k = child_off[i]; k < child_off[i + 1]; ++k)
			if (child_idx[k] <= i || child_idx[k] >= n_nodes) return fail(MCS_ERR_INVALID, "children must have larger node ids than their parent (DBoW2 numbers nodes top-down)");
	}
	HIPCHK(hipSetDevice(c->device));
	mcs_vocabulary* v = new mcs_vocabulary();
	v->ctx = c; v->nNodes = n_nodes; v->L = L;
	Staging stg(c, true);
	stg.upload(&v->nodeDesc, node_desc, (size_t)n_nodes * 32); stg.upload(&v->childOff, child_off, ((size_t)n_nodes + 1) * 4);
	stg.upload(&v->childIdx, child_idx, (size_t)child_off[n_nodes] * 4);
	const bool ok = v->tree.reserve(stg.bytes()) == hipSuccess && stg.commit(v->tree.p) == MCS_OK;
	if (stg.finish(ok ? MCS_OK : MCS_ERR_HIP) != MCS_OK) { delete v; return fail(MCS_ERR_HIP, "vocabulary upload failed"); }
	*out = v;
	return MCS_OK;
}

void mcs_vocabulary_destroy(mcs_vocabulary* v) {
	if (!v) return;
	(void)hipSetDevice(v->ctx->device);
	delete v;
}

int mcs_bow_transform(mcs_vocabulary* v, const uint8_t* desc, int n, int stride, int levelsup, mcs_mem_kind kind, int32_t* leaf_node, int32_t* node_at_level) {
	if (!v || !desc || !leaf_node || !node_at_level) return fail(MCS_ERR_INVALID, "null argument");
	if (n < 0 || stride < 32 || (stride & 3)) return fail(MCS_ERR_INVALID, "descriptors must be >= 32 bytes per row (FORB compares 32 bytes), stride a multiple of 4");
	if (n == 0) return MCS_OK;
	mcs_ctx* c = v->ctx;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t s = c->stream;
	BowArgs a{v->nodeDesc, v->childOff, v->childIdx, v->L, nullptr, n, stride, levelsup, nullptr, nullptr};
	Staging st(c, kind == MCS_MEM_HOST);
	st.in(&a.desc, desc, (size_t)n * stride); st.out(&a.leaf, leaf_node, (size_t)n * 4); st.out(&a.nid, node_at_level, (size_t)n * 4);
	if (int r = st.commit()) return r;
	hipLaunchKernelGGL(k_bow_transform, dim3((n + 255) / 256), dim3(256), 0, s, a);
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) return fail(MCS_ERR_HIP, std::string("bow transform: ") + hipGetErrorString(e));
	return st.finish(MCS_OK);
}

int mcs_bow_vector(mcs_vocabulary* v, const int32_t* leaf_nodes, int n, mcs_mem_kind kind, int32_t* word_ids_out, double* values_out, int32_t* nwords_out) {
	if (!v || n < 0 || (n && (!leaf_nodes || !word_ids_out || !values_out)) || !nwords_out) return fail(MCS_ERR_INVALID, "null argument");
	if (!v->wordOf) return fail(MCS_ERR_INVALID, "mcs_bow_vector: call mcs_vocabulary_set_words first");
	mcs_ctx* c = v->ctx;
	HIPCHK(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	const bool host = kind == MCS_MEM_HOST;
	const size_t nn = std::max(n, 1);
	// host kind: the outputs hold nwords_out entries, known only after the kernel, so they are fetched below from the block (intact until the next call)
	const int* dLeaf = nullptr; int *dW = nullptr, *outW = nullptr, *nOut = nullptr, *dErr = nullptr; double *dWt = nullptr, *outV = nullptr;
	int errv = 0, d = 0;
	Staging stg(c, host);
	stg.in(&dLeaf, leaf_nodes, (size_t)n * 4); stg.scratch(&dW, nn * 4); stg.scratch(&dWt, nn * 8); stg.download(&dErr, &errv, 4);
	if (host) { stg.scratch(&outW, nn * 4); stg.scratch(&outV, nn * 8); stg.download(&nOut, &d, 4); }
	else { outW = word_ids_out; outV = values_out; nOut = nwords_out; }
	if (int r = stg.commit()) return r;
	HIPCHK(hipMemsetAsync(dErr, 0, 4, st));
	hipLaunchKernelGGL(k_bow_vector, dim3(1), dim3(1024), 0, st, dLeaf, n, v->nNodes, v->nWords, v->wordOf, v->weightOf, v->hist, dW, dWt, outW, outV, nOut, dErr);
	HIPCHK(hipGetLastError());
	if (int r = stg.finish(MCS_OK)) return r;
	if (errv & 1) return fail(MCS_ERR_INVALID, "mcs_bow_vector: leaf node id out of range");
	if (errv & 2) return fail(MCS_ERR_INVALID, "mcs_bow_vector: a node with a weight > 0 has no word id (not a leaf)");
	if (host) {
		*nwords_out = d;
		if (d) {
			HIPCHK(hipMemcpyAsync(word_ids_out, outW, (size_t)d * 4, hipMemcpyDeviceToHost, st));
			HIPCHK(hipMemcpyAsync(values_out, outV, (size_t)d * 8, hipMemcpyDeviceToHost, st));
			HIPCHK(hipStreamSynchronize(st));
		}
	}
	return MCS_OK;
}
