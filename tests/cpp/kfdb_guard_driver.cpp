// kfdb_guard_driver.cpp — runs the BowVector CSR checks of the keyframe database (csrc/mcs_kfdb_guard.hip) the way mcs_kfdb_add calls them (offsets as a whole,
// then the words they delimit) and prints one line per case: name, code, text (tab-separated).  The word array of a case is exactly as long as its last offset
// says when the offsets are good, and SHORTER than an earlier offset claims in the cases where they are bad: a check that walked the words by unchecked offsets
// would read past it (the driver is built with the host sanitizers where they link).  No HIP call; tests/test_kfdb_guards_cpu.py.
#include "mcs_host.h"

#include <cstdio>

std::string& mcs_err() { static std::string e; return e; }   // the library's is in mcs_capi.hip

static const char* const WHAT = "mcs_kfdb_add";

// what mcs_kfdb_add does between fetching the offsets and touching the database; the words are copied to a heap block of exactly words.size() ints
static int add_checks(const std::vector<int>& off, const std::vector<int>& words, int nWords, const char* what = WHAT) {
	const int n = (int)off.size() - 1;
	if (int r = guard_bow_offsets(off.data(), n, what)) return r;
	if ((size_t)off[n] != words.size()) return -99;   // a mistake of the case, not of the guard
	int* w = new int[words.size()];                   // exactly: any read past it (new int[0]: any read at all) is the sanitizer's to report
	std::copy(words.begin(), words.end(), w);
	const int rc = guard_bow_words(off.data(), n, w, nWords, what);
	delete[] w;
	return rc;
}

static void run(const char* name, const std::vector<int>& off, const std::vector<int>& words, int nWords, const char* what = WHAT) {
	mcs_err().clear();
	const int rc = add_checks(off, words, nWords, what);
	printf("%s\t%d\t%s\n", name, rc, rc ? mcs_err().c_str() : "");
}

int main() {
	const int NW = 100;
	run("ok", {0, 3, 5}, {0, 31, 99, 32, 33}, NW);
	run("ok.nkf0", {0}, {}, NW);
	run("ok.empty_rows_between", {0, 2, 2, 2, 4, 4}, {1, 2, 1, 2}, NW);
	run("ok.all_rows_empty", {0, 0, 0}, {}, NW);
	run("ok.one_word_vocabulary", {0, 1}, {0}, 1);
	run("offsets.first_above_0", {1, 2}, {5, 6}, NW);
	run("offsets.decrease_after_large_row", {0, 10, 4}, {1, 2, 3, 4}, NW);   // row 0 claims w[0..10) of four words
	run("offsets.negative_last", {0, -1}, {}, NW);
	run("offsets.negative_last_after_rows", {0, 2, -1}, {1, 2}, NW);
	run("offsets.bare_text", {0, 3, 2}, {1, 2}, NW, nullptr);
	run("word.equals_n_words", {0, 2}, {5, 100}, NW);
	run("word.minus_1", {0, 2}, {-1, 5}, NW);
	run("word.equal_neighbours", {0, 3}, {4, 7, 7}, NW);
	run("word.descending_pair", {0, 3}, {4, 9, 8}, NW);
	run("word.descending_across_rows_is_fine", {0, 2, 4}, {8, 9, 1, 2}, NW);
	run("word.other_entry_point", {0, 2}, {7, 7}, NW, "mcs_kfdb_score");
	// collisions: which check answers first
	run("first_above_0+decrease", {2, 1}, {5}, NW);
	run("decrease+bad_word_in_earlier_row", {0, 2, 1}, {500}, NW);           // the offsets are judged before any word is read
	run("range+order_at_one_word", {0, 2}, {50, -3}, NW);                     // -3 is out of range AND below its neighbour: the range answers
	run("order_in_row_0+range_in_row_1", {0, 2, 3}, {9, 9, 100}, NW);        // rows in order
	run("range_in_row_0+order_in_row_1", {0, 1, 3}, {100, 9, 9}, NW);
	return 0;
}
