// vr_devbvh.hpp -- the device BVH builder (vr_devbvh.hip): a Morton-ordered,
// count-balanced tree built from device-resident triangles straight into the
// eight arrays of the device mesh layout (vr_mesh_layout.hpp DeviceMesh).  No
// reference counterpart: the reference builds on the host (src/SBVH.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "vr_devmesh.hpp"

namespace vr {

// Closed-form shape of the tree for n_tris triangles (see vr_devbvh.hip).
struct DevBuildShape {
    uint32_t n_refs;     // compact triangles: n_tris, or 2 for a single triangle (stored twice)
    uint32_t leaves;     // L = max(2, ceil(n_refs / max_leaf))
    uint32_t nodes;      // L - 1
    uint32_t depth;      // ceil(log2 L)
};
inline DevBuildShape devbvh_shape(uint32_t n_tris, uint32_t max_leaf)
{
    DevBuildShape s;
    s.n_refs = n_tris < 2u ? 2u : n_tris;
    const uint32_t l = (s.n_refs + max_leaf - 1u) / max_leaf;
    s.leaves = l < 2u ? 2u : l;
    s.nodes = s.leaves - 1u;
    s.depth = 0u;
    while ((1ull << s.depth) < s.leaves) ++s.depth;
    return s;
}

// Enqueues the whole build on `stream`.  All pointers are device pointers;
// normals, tangents and uvs may be null (zeros).  *scratch_out is the build's
// scratch arena: the caller frees it (hipFree) once the stream has finished.
// d_status must be zero-filled on the stream before the call.  Returns 0, or
// a hipError_t; on an error *scratch_out is already freed (null).
int devbvh_build(const float* positions, const float* normals, const float* tangents, const float* uvs,
                 uint32_t n_verts, const uint32_t* tris, uint32_t n_tris, uint32_t max_leaf,
                 const MeshArrays& out, DevBuildStatus* d_status, void** scratch_out, void* stream);

} // namespace vr
