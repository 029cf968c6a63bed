// vr_devbvh.hpp -- the device BVH builder (vr_devbvh.hip): a Morton-ordered,
// count-balanced tree built from device-resident triangles straight into the
// eight arrays of the device mesh layout (vr_mesh_layout.hpp DeviceMesh).  No
// reference counterpart: the reference builds on the host (src/SBVH.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "vr_params.hpp"

namespace vr {

#if defined(__HIPCC__)
#define VR_DEVBVH_HD __host__ __device__
#else
#define VR_DEVBVH_HD
#endif

// IEEE binary16 bits of the float with bit pattern `bits`, rounded toward
// +inf (up) or -inf (down); equals half_bits_directed (vr_mesh_layout.cpp) for
// every non-NaN float (both infinities included; NaN patterns differ, see
// docs/DESIGN_HISTORY.md).  The magnitude is truncated toward zero and stepped one
// half ulp outward when that moved it to the wrong side: 0x7bff + 1 is
// infinity (out of range on the outward side), 0x03ff + 1 the smallest normal.
VR_DEVBVH_HD inline uint16_t half_directed(uint32_t bits, bool up)
{
    const uint32_t sign = (bits >> 16) & 0x8000u;
    const uint32_t a = bits & 0x7fffffffu;
    uint32_t mag;
    bool inexact;
    if (a >= 0x477fe000u) {                       // |x| >= 65504: the largest finite half
        mag = 0x7bffu;
        inexact = a > 0x477fe000u;
    } else if (a < 0x38800000u) {                 // |x| < 2^-14: half subnormal, |x| * 2^24 truncated
        const uint32_t e = a >> 23;
        const uint32_t mant = (a & 0x7fffffu) | 0x800000u;
        const uint32_t sh = 126u - e;             // >= 14
        if (e == 0u || sh > 24u) { mag = 0u; inexact = a != 0u; }
        else { mag = mant >> sh; inexact = (mant & ((1u << sh) - 1u)) != 0u; }
    } else {                                      // normal: rebias the exponent, keep 10 fraction bits
        mag = (a - 0x38000000u) >> 13;
        inexact = (a & 0x1fffu) != 0u;
    }
    if (inexact && (up != (sign != 0u))) mag += 1u;   // outward: away from zero on the rounding side
    return (uint16_t)(sign | mag);
}

enum : uint32_t { DEVBVH_BAD_INDEX = 1u, DEVBVH_NONFINITE = 2u };

// the record the build leaves for the host (one small read-back)
struct DevBuildStatus {
    uint32_t flags;      // DEVBVH_* errors found on the device
    uint32_t depth;      // as validate_flat counts it (root = 1)
    uint32_t nodes;      // inner nodes
    uint32_t leaves;
    uint32_t slots;      // reference slots: 3 per triangle reference + 1 terminator per leaf
    uint32_t pad[3];
};

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

// the eight arrays of the device mesh, allocated by the caller for `shape`:
// bvh float4[4 nodes], bvh16 float4[2 nodes], verts / tri_e vr3[3 n_refs],
// tpath u64[n_refs], normals / tangents float4[3 n_refs], uvs vr2[3 n_refs];
// and what a refit needs (vr_refit.hpp): slot_vert u32[3 n_refs], the caller's
// vertex index behind each compact vertex slot, and node_level u32[nodes], each
// node's level in the emitted order (the root 0; refit_levels)
struct DevBuildOut {
    vr4* bvh; vr4* bvh16; vr3* verts; vr3* tri_e; unsigned long long* tpath;
    vr4* normals; vr4* tangents; vr2* uvs; uint32_t* slot_vert; uint32_t* node_level;
};

// Enqueues the whole build on `stream`.  All pointers are device pointers;
// normals, tangents and uvs may be null (zeros).  *scratch_out is the build's
// scratch arena: the caller frees it (hipFree) once the stream has finished.
// d_status must be zero-filled on the stream before the call.  Returns 0, or
// a hipError_t; on an error *scratch_out is already freed (null).
int devbvh_build(const float* positions, const float* normals, const float* tangents, const float* uvs,
                 uint32_t n_verts, const uint32_t* tris, uint32_t n_tris, uint32_t max_leaf,
                 const DevBuildOut& out, DevBuildStatus* d_status, void** scratch_out, void* stream);

// half_directed on n device floats, both directions (vrhip_selftest_half_box)
int launch_half_box(const float* in, size_t n, uint16_t* down, uint16_t* up, void* stream);

} // namespace vr
