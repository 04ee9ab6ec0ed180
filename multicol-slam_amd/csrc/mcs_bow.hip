// mcs_bow.hip — cMultiFrame::ComputeBoW (src/cMultiFrame.cpp:356-363): the DBoW2 vocabulary-tree descent of every descriptor
// (ThirdParty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1259 with FORB::distance, FORB.cpp:85-105), SURVEY §8f row 4.
// One lane per feature: the descriptor (32 bytes, what FORB compares) sits in 8 VGPRs, every level reads the <= k child descriptors of the
// current node (the small vocabulary — 8823 nodes x 32 B — stays in L2) and keeps the first strict minimum, like the reference.
// Outputs per feature: the leaf node reached and the node of the path at level L - levelsup; word ids, weights and the BowVector /
// FeatureVector maps are table look-ups and a sort on the host.
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

}  // namespace mcs

using namespace mcs;

struct mcs_vocabulary {
	mcs_ctx* ctx = nullptr;
	int nNodes = 0, L = 0;
	uint8_t* nodeDesc = nullptr; int* childOff = nullptr; int* childIdx = nullptr;
	// word id and weight of every node (mcs_vocabulary_set_words) and a zeroed per-word histogram for mcs_bow_vector (mcs_kfdb.hip)
	int nWords = 0; int* wordOf = nullptr; double* weightOf = nullptr; int* hist = nullptr;
};

int mcs_vocabulary_set_words_internal(mcs_vocabulary* v, const int32_t* word_id_per_node, const double* weight_per_node) {
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
	HIPCHK(hipSetDevice(v->ctx->device));
	(void)hipFree(v->wordOf); (void)hipFree(v->weightOf); (void)hipFree(v->hist);
	v->wordOf = nullptr; v->weightOf = nullptr; v->hist = nullptr; v->nWords = 0;
	const size_t nn = (size_t)v->nNodes, nw = (size_t)std::max(mx + 1, 1);
	bool ok = hipMalloc((void**)&v->wordOf, nn * 4) == hipSuccess && hipMalloc((void**)&v->weightOf, nn * 8) == hipSuccess &&
	          hipMalloc((void**)&v->hist, nw * 4) == hipSuccess;
	ok = ok && hipMemcpy(v->wordOf, word_id_per_node, nn * 4, hipMemcpyHostToDevice) == hipSuccess &&
	     hipMemcpy(v->weightOf, weight_per_node, nn * 8, hipMemcpyHostToDevice) == hipSuccess && hipMemset(v->hist, 0, nw * 4) == hipSuccess;
	if (!ok) return fail(MCS_ERR_HIP, "vocabulary word upload failed");
	v->nWords = (int)nw;
	return MCS_OK;
}

int mcs_vocabulary_words_internal(mcs_vocabulary* v, mcs_ctx** c, int* nNodes, int** wordOf, double** weightOf, int** hist, int* nWords) {
	if (!v->wordOf) return fail(MCS_ERR_INVALID, "mcs_bow_vector: call mcs_vocabulary_set_words first");
	*c = v->ctx; *nNodes = v->nNodes; *wordOf = v->wordOf; *weightOf = v->weightOf; *hist = v->hist; *nWords = v->nWords;
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
	const size_t nidx = (size_t)child_off[n_nodes];
	bool ok = hipMalloc((void**)&v->nodeDesc, (size_t)n_nodes * 32) == hipSuccess && hipMalloc((void**)&v->childOff, ((size_t)n_nodes + 1) * 4) == hipSuccess &&
	          hipMalloc((void**)&v->childIdx, std::max<size_t>(nidx, 1) * 4) == hipSuccess;
	ok = ok && hipMemcpy(v->nodeDesc, node_desc, (size_t)n_nodes * 32, hipMemcpyHostToDevice) == hipSuccess &&
	     hipMemcpy(v->childOff, child_off, ((size_t)n_nodes + 1) * 4, hipMemcpyHostToDevice) == hipSuccess &&
	     hipMemcpy(v->childIdx, child_idx, nidx * 4, hipMemcpyHostToDevice) == hipSuccess;
	if (!ok) { mcs_vocabulary_destroy(v); return fail(MCS_ERR_HIP, "vocabulary upload failed"); }
	*out = v;
	return MCS_OK;
}

void mcs_vocabulary_destroy(mcs_vocabulary* v) {
	if (!v) return;
	(void)hipFree(v->nodeDesc); (void)hipFree(v->childOff); (void)hipFree(v->childIdx);
	(void)hipFree(v->wordOf); (void)hipFree(v->weightOf); (void)hipFree(v->hist);
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
