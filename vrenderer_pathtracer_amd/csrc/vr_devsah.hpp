// vr_devsah.hpp -- the device binned-SAH builder (vr_devsah.hip): the tree
// vr::build_flat builds on the host (vr_bvh.cpp Builder::build: object splits,
// 128 bins per axis), built level by level on the device from device-resident
// triangles into the eight arrays of the device mesh layout.
//
// Every decision of the host builder is a function of min/max boxes, integer
// counts and fp64 arithmetic on those, so it does not depend on the order in
// which references are visited; the one order-dependent step, the partition,
// is stable here, which fixes each leaf's triangles in ascending input index.
// The arithmetic of those decisions lives in this header as VR_DEVBVH_HD
// functions: the kernels and a host driver (tests/sah_driver.cpp) compile the
// same text.  The library is compiled with -ffp-contract=off, as vr_bvh.cpp is.
//
// VRHIP_SAH_NODE_COST and VRHIP_SBVH_ALPHA are experiment switches of the host
// builder; this builder ignores them (node cost 1, no spatial splits).
#pragma once
#include <cstddef>
#include <cstdint>

#include "vr_bvh.hpp"
#include "vr_devmesh.hpp"

namespace vr {

constexpr int kSahBins = 128;                     // vr_bvh.cpp VR_BVH_BINS
// Nodes of at most kSahSmall references are handled by one wave64 in
// registers (a lane per reference); larger nodes bin into global memory.
constexpr uint32_t kSahSmall = 64;

using SahBox = DevBox;                            // the layout is shared, sah_grow is this builder's own
VR_DEVBVH_HD inline SahBox sah_empty() { return empty_box(); }
// Box::grow (vr_bvh.cpp:34-39): componentwise min / max
VR_DEVBVH_HD inline void sah_grow(SahBox& b, const SahBox& o)
{
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = o.lo[a] < b.lo[a] ? o.lo[a] : b.lo[a];
        b.hi[a] = o.hi[a] > b.hi[a] ? o.hi[a] : b.hi[a];
    }
}
// the centroid of a triangle box (vr_bvh.cpp:464): 0.5f * (lo + hi) in fp32
VR_DEVBVH_HD inline float sah_centroid(float lo, float hi) { return 0.5f * (lo + hi); }

// Box::area (vr_bvh.cpp:41-45): the differences in fp64 from the fp32 bounds
VR_DEVBVH_HD inline double sah_area(const SahBox& b)
{
    if (b.lo[0] > b.hi[0]) return 0.0;
    const double dx = (double)b.hi[0] - b.lo[0], dy = (double)b.hi[1] - b.lo[1], dz = (double)b.hi[2] - b.lo[2];
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}
// the bin of centroid c on an axis whose centroid bounds start at lo and span
// ext > 0 (vr_bvh.cpp Builder::bin_of and its two callers)
VR_DEVBVH_HD inline int sah_bin(float c, float lo, float ext)
{
    const double scale = kSahBins / (double)ext;
    const double x = ((double)c - lo) * scale;
    int k = x == x ? (int)x : 0;                  // NaN (an overflowed centroid, scale 0): bin 0, as Builder::bin_of
    k = k < 0 ? 0 : k;
    return k > kSahBins - 1 ? kSahBins - 1 : k;
}
// the cost of a candidate (vr_bvh.cpp:175); both counts are > 0
VR_DEVBVH_HD inline double sah_cost(double area_l, uint32_t n_l, double area_r, uint32_t n_r)
{
    return area_l * n_l + area_r * n_r;
}
// The host sweeps axes 0, 1, 2 and bins ascending and keeps the first strict
// minimum (vr_bvh.cpp:161-178).  A candidate's key is axis * kSahBins + bin;
// an argmin in any order gives the host's winner when ties go to the lower key.
VR_DEVBVH_HD inline uint32_t sah_key(int axis, int k) { return (uint32_t)(axis * kSahBins + k); }
constexpr uint32_t kSahNoKey = 0xffffffffu;
VR_DEVBVH_HD inline bool sah_better(double cost, uint32_t key, double best_cost, uint32_t best_key)
{
    return cost < best_cost || (cost == best_cost && key < best_key);
}
// vr_bvh.cpp:144: a leaf before any binning (the root is always split)
VR_DEVBVH_HD inline bool sah_early_leaf(uint32_t count, uint32_t depth, bool root)
{
    return !root && (count <= 1u || depth + 1u >= kMaxBuildDepth);
}
// vr_bvh.cpp:179-183: leaf or split, once the best candidate is known
VR_DEVBVH_HD inline bool sah_want_leaf(uint32_t count, uint32_t max_leaf, bool has_axis, double best_cost,
                                       double parent_area)
{
    const double split_cost = 1.0 + (parent_area > 0.0 ? best_cost / parent_area : (double)count);
    return count <= max_leaf && (!has_axis || split_cost >= (double)count);
}
// vr_bvh.cpp:196: coincident centroids split the current order in the middle
VR_DEVBVH_HD inline uint32_t sah_median(uint32_t count) { return count / 2u; }

// An order-preserving integer image of a float (signed compare), its own
// inverse: the kernels take min / max of boxes with integer atomics.
VR_DEVBVH_HD inline int32_t sah_ordered(int32_t bits) { return bits >= 0 ? bits : bits ^ 0x7fffffff; }

// the child's root path under a leading 1 (vr_mesh_layout.cpp tri_paths):
// `path` is the parent's, whose leading 1 is at bit `depth`
VR_DEVBVH_HD inline unsigned long long sah_child_path(unsigned long long path, uint32_t depth, uint32_t ch)
{
    return (path ^ (1ull << depth)) | ((unsigned long long)ch << depth) | (1ull << (depth + 1u));
}

// Scratch the build takes for n_refs references, in bytes.
size_t devsah_arena_bytes(uint32_t n_tris);

// As devbvh_build (vr_devbvh.hpp), with two differences: `out` must hold
// n_refs - 1 nodes (the worst case; d_status->nodes is the real count), and
// the call reads back one counter per tree level, so the build has finished
// when it returns.  d_status->depth is the tree's real depth.
int devsah_build(const float* positions, const float* normals, const float* tangents, const float* uvs,
                 uint32_t n_verts, const uint32_t* tris, uint32_t n_tris, uint32_t max_leaf,
                 const MeshArrays& out, DevBuildStatus* d_status, void** scratch_out, void* stream);

} // namespace vr
