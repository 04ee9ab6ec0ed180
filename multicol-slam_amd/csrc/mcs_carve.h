// mcs_carve.h — layout of aligned pieces in one block: plain C++, no runtime calls (tests/test_carve_cpu.py compiles it on its own).
#pragma once
#include <cstddef>

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

// Offsets of aligned pieces in one block: take() in the order of declaration, `total` is the block's size.  No runtime calls.
struct Carve {
	size_t total = 0;
	size_t take(size_t bytes) { const size_t at = total; total += al256(bytes > 0 ? bytes : 1); return at; }
};
