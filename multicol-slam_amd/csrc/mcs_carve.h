// mcs_carve.h — layout of aligned pieces in one block: plain C++, no runtime calls (tests/test_carve_cpu.py compiles it on its own).
#pragma once
#include <cstddef>
#include <vector>

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

// Offsets of aligned pieces in one block: take() in the order of declaration, `total` is the block's size.  No runtime calls.
struct Carve {
	size_t total = 0;
	size_t take(size_t bytes) { const size_t at = total; total += al256(bytes > 0 ? bytes : 1); return at; }
};

// Carve with the pointers bound, for a block whose address is known only after its size: piece() takes the room in the order of declaration and records the
// pointer, place() assigns every recorded pointer.  To Carve what Staging::scratch is to Staging.  A null pointer-to-bind takes the room and binds nothing
// (a piece that one variant of a call does not use keeps its place, so the layout does not depend on the variant).
struct Layout : Carve {
	struct Bound { void** p; size_t off; };
	std::vector<Bound> bound;
	template <class P> void piece(P** p, size_t bytes) {
		const size_t at = take(bytes);
		if (p) bound.push_back(Bound{(void**)p, at});
	}
	void place(unsigned char* base) const { for (const Bound& b : bound) *b.p = base + b.off; }
};
