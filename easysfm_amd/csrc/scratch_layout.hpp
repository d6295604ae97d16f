// Layout arithmetic of the stages' scratch buffers, free of HIP so that the *_check.hpp headers and their g++ programs under
// tests/cpp share it with the entry points.
#pragma once

#include <cstddef>
#include <cstdint>

namespace esfm {

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// bits needed to write x: a radix sort over keys below 2^bit_width(bound) ends at that bit
inline int bit_width(uint64_t x) { int n = 0; while (x) { ++n; x >>= 1; } return n; }

// Carves one buffer into arrays that each start on a multiple of 256 bytes: take() returns the array's byte offset, `at` is the
// size of the buffer so far.
struct ScratchCarver {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t here = at; at += align256(bytes); return here; }
};

}  // namespace esfm
