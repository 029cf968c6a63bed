// vr_devmesh.hpp -- what the device builders (vr_devbvh.hip, vr_devsah.hip)
// and the refit (vr_refit.hip) share about the device mesh layout
// (vr_mesh_layout.hpp DeviceMesh): the status record, the mesh's arrays, the
// leaf code, the box and the fp16 rounding of the node rows.  Host-compilable:
// tests/half_driver.cpp and tests/sah_driver.cpp compile this text.  The
// device side is vr_devmesh_dev.hpp and vr_devmesh.hip.
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

// A sum of doubles carried as an unevaluated pair hi + lo (|lo| <= ulp(hi) / 2)
// with error-free additions (Knuth's TwoSum), the running error below 2^-100
// of the sum: rounded to one double, the sum of a few thousand positive terms
// depends on the order they were added in only where it lies within that
// 2^-100 of a rounding boundary, which no test has met and nothing rules out.
// The SAH cost is summed this way by the host (vr_bvh.cpp flat_sah_cost) and by
// the device (vr_refit.hip), which walk the nodes in different orders and are
// compared by bits (tests/test_gpu_extreme.py).  Needs -ffp-contract=off and no fast-math, as the library has.
struct Sum2 { double hi = 0.0, lo = 0.0; };
VR_DEVBVH_HD inline void sum2_add(Sum2& s, double x_hi, double x_lo = 0.0)
{
    const double t = s.hi + x_hi;
    const double b = t - s.hi;
    const double e = ((s.hi - (t - b)) + (x_hi - b)) + (s.lo + x_lo);
    s.hi = t + e;
    s.lo = e - (s.hi - t);
}

// half_directed on n device floats, both directions (vrhip_selftest_half_box)
int launch_half_box(const float* in, size_t n, uint16_t* down, uint16_t* up, void* stream);

// errors found on the device (DevBuildStatus::flags)
enum : uint32_t { DEVBVH_BAD_INDEX = 1u, DEVBVH_NONFINITE = 2u, DEVBVH_BIG_LEAF = 4u, DEVBVH_INTERNAL = 8u };

// the record a build or a refit leaves for the host (one small read-back)
struct DevBuildStatus {
    uint32_t flags;      // DEVBVH_*
    uint32_t depth;      // as validate_flat counts it (root = 1)
    uint32_t nodes;      // inner nodes
    uint32_t leaves;
    uint32_t slots;      // reference slots: 3 per triangle reference + 1 terminator per leaf
    uint32_t pad[3];
};

// The one description of a device mesh's arrays (device pointers; the host's
// resident mesh owns them, vr_ctx.hpp ResidentMesh).  The eight the path
// kernels read: bvh float4[4 n_nodes], bvh16 float4[2 n_nodes], verts / tri_e
// vr3[3 n_refs], tpath u64[n_refs], normals / tangents float4[3 n_refs], uvs
// vr2[3 n_refs].  What a refit needs (vr_refit.hpp; null after a host upload):
// slot_vert u32[3 n_refs], the caller's vertex index behind each compact
// vertex slot, and node_level u32[n_nodes], each node's level in the emitted
// order (the root 0; refit_levels).  What a ray query reports
// (vr_rayquery.hpp): prim_id u32[n_refs], the caller's triangle of each
// compact triangle after a device build, the flat slot of its first vertex
// after a host upload.
// The shape: nodes and compact triangles in use, and the tree's depth as
// DevBuildStatus counts it.  The builders fill arrays sized for their worst
// case and report the shape through DevBuildStatus: they ignore these three.
struct MeshArrays {
    vr4* bvh; vr4* bvh16; vr3* verts; vr3* tri_e; unsigned long long* tpath;
    vr4* normals; vr4* tangents; vr2* uvs; uint32_t* slot_vert; uint32_t* node_level;
    uint32_t* prim_id;
    uint32_t n_nodes, n_refs, depth;
};

// A leaf child's index word: ~((first << 7) | count) over the compact triangles
// (vr_kernel.hpp trav_iter reads it); an inner child's is its float4 offset.
VR_DEVBVH_HD inline bool leaf_count_fits(uint32_t count) { return (count >> kLeafCountBits) == 0u; }
VR_DEVBVH_HD inline int32_t leaf_code(uint32_t first, uint32_t count)
{
    return ~(int32_t)((first << kLeafCountBits) | count);
}
VR_DEVBVH_HD inline void leaf_range(int32_t code, uint32_t& first, uint32_t& count)
{
    const uint32_t u = (uint32_t)~code;
    first = u >> kLeafCountBits;
    count = u & ((1u << kLeafCountBits) - 1u);
}

// One box layout for every device-side site.  How a box grows is not shared:
// the SAH builder selects with < and > as the host's Box::grow does
// (vr_devsah.hpp sah_grow), the Morton builder and the refit use fminf / fmaxf
// (vr_devmesh_dev.hpp grow_fminmax); the two can differ in the sign of a zero bound.
struct DevBox { float lo[3], hi[3]; };

VR_DEVBVH_HD inline DevBox empty_box()
{
    const float inf = __builtin_inff();
    return { { inf, inf, inf }, { -inf, -inf, -inf } };
}

} // namespace vr
