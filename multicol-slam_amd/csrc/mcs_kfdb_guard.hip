// mcs_kfdb_guard.hip — the checks of a BowVector CSR (offsets[n+1], ascending word ids per row) as mcs_kfdb_add, mcs_kfdb_detect_* and mcs_kfdb_score take
// it.  No HIP call in this file.  The offsets are checked as a whole before a caller sizes or fetches anything by them; the words only after that.
#include "mcs_host.h"

// `what` names the entry point in front of the text; null: the bare text (the detection calls check their offsets before they know the form)
static int refuse(const char* what, const char* text) { return fail(MCS_ERR_INVALID, what ? std::string(what) + ": " + text : std::string(text)); }

int guard_bow_offsets(const int* off, int n, const char* what) {
	if (off[0] != 0) return fail(MCS_ERR_INVALID, "offsets[0] must be 0");
	for (int i = 0; i < n; ++i)
		if (off[i + 1] < off[i]) return refuse(what, "offsets must be non-decreasing");
	return MCS_OK;
}

// off has passed guard_bow_offsets and w holds off[n] words
int guard_bow_words(const int* off, int n, const int* w, int nWords, const char* what) {
	for (int i = 0; i < n; ++i)
		for (int k = off[i]; k < off[i + 1]; ++k) {
			if (w[k] < 0 || w[k] >= nWords) return refuse(what, "word id out of range");
			if (k > off[i] && w[k - 1] >= w[k]) return refuse(what, "word ids of a BowVector must be strictly ascending");
		}
	return MCS_OK;
}
