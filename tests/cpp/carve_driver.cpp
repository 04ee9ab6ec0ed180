// The block layout of the host-kind staging (csrc/mcs_carve.h): pieces given on the command line -> "offset size" per piece and the total; then the same
// pieces through the binding layout: "offset" per piece as its bound pointer reads once the block is placed, and the total.
#include "mcs_carve.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
	Carve cv;
	for (int i = 1; i < argc; ++i) {
		const size_t before = cv.total, at = cv.take((size_t)strtoull(argv[i], nullptr, 10));
		if (at != before) return 1;
		printf("%zu %zu\n", at, cv.total - at);
	}
	printf("%zu\n", cv.total);
	Layout lay;
	std::vector<const char*> bound(argc, nullptr);   // pointers of another type than the block's: piece() binds any
	for (int i = 1; i < argc; ++i) lay.piece(&bound[i], (size_t)strtoull(argv[i], nullptr, 10));
	lay.piece((int**)nullptr, 100);                  // room without a pointer: moves the total, binds nothing
	for (int i = 1; i < argc; ++i)
		if (bound[i]) return 2;                      // nothing is bound before place()
	unsigned char* const base = (unsigned char*)(size_t)0x10000;   // never dereferenced
	lay.place(base);
	for (int i = 1; i < argc; ++i) printf("%zu\n", (size_t)((const unsigned char*)bound[i] - base));
	printf("%zu\n", lay.total);
	return 0;
}
