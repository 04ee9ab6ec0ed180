// The block layout of the host-kind staging (csrc/mcs_carve.h): pieces given on the command line -> "offset size" per piece and the total.
#include "mcs_carve.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
	Carve cv;
	for (int i = 1; i < argc; ++i) {
		const size_t before = cv.total, at = cv.take((size_t)strtoull(argv[i], nullptr, 10));
		if (at != before) return 1;
		printf("%zu %zu\n", at, cv.total - at);
	}
	printf("%zu\n", cv.total);
	return 0;
}
