// The argument check the mesh entry points share (esfm_mesh_components, esfm_mesh_clean, esfm_mesh_simplify), free of HIP so that
// simplify_check.hpp stays buildable with g++ alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "error.hpp"

namespace esfm {

// The ranges of the two counts and every triangle index, on the caller's copy.  Reads, writes nothing.
inline int check_mesh(int V, int T, const int32_t *triangles)
{
    ESFM_REQUIRE(V >= 0 && V <= (1 << 30), "n_vertices must be 0..2^30");
    ESFM_REQUIRE(T >= 0 && T <= (1 << 28), "n_triangles must be 0..2^28");
    ESFM_REQUIRE(T == 0 || triangles, "NULL argument");
    for (size_t i = 0; i < 3 * (size_t)T; ++i) ESFM_REQUIRE(triangles[i] >= 0 && triangles[i] < V, "a triangle index is outside 0..n_vertices-1");
    return ESFM_OK;
}

}  // namespace esfm
