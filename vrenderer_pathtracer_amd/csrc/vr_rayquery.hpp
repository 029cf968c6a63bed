// vr_rayquery.hpp -- closest-hit and any-hit ray queries against the triangle
// mesh (vrhip_trace_rays, vrhip_flat_trace_rays): the device kernel's launcher
// (vr_rayquery.hip) and the host walk over the flattened reference layout
// (vr_raycast.cpp), the yardstick of the kernel.  No reference counterpart as
// a call: the reference traces its own camera and bounce rays only; the walk
// and the triangle test are its own (cuda/src/PathTracer.cu:276-463,
// cuda/include/RayIntersection.cuh:54-111).  Plain C++: a sanitizer driver
// compiles vr_raycast.cpp with this header (tests/raycast_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vr_params.hpp"

namespace vr {

constexpr uint32_t kRayMiss = 0xffffffffu;        // VRHIP_RAY_MISS
constexpr float kRayNoHit = 1e20f;                // the reference's "no hit" distance (PathTracer.cu:145)
enum : uint32_t { RAYS_CLOSEST = 0u, RAYS_ANY = 1u };
struct alignas(4) RayHit { float t; uint32_t prim; float u, v; };   // vrhip_ray_hit

// One launch of the query kernel; every pointer is a device pointer.
struct RayQuery {
    const float* origins;        // float[3 n_rays]
    const float* dirs;           // float[3 n_rays], used as given
    const float* tmax;           // float[n_rays] or nullptr (kRayNoHit)
    uint32_t n_rays;
    uint32_t any_hit;            // 1: hit or miss only, the walk ends at the first accepted triangle
    const uint32_t* prim_id;     // per compact triangle, what RayHit::prim reports
    RayHit* hits;                // [n_rays], 16-byte aligned
};

// p: bvh, bvh16, tri_e, tpath, n_nodes, n_tris and flags (F_MESH, F_STRICT for
// the strict walk) are read.  stack: 16, 24, 32 or 64 entries (tree depth + 1
// at least).  Enqueues on `stream`; 0 or a hipError_t.  n_rays > 0.
int launch_ray_query(const RenderParams& p, const RayQuery& q, int stack, uint32_t cu_count, void* stream);

// The host walk: the reference's per-lane traversal over the flattened arrays
// (every pierced box, near child first and child 0 on equal entries, leaf
// slots in order up to the terminator, strict < on the closest-hit update), in
// fp32 without contraction.  RayHit::prim is the slot of the hit triangle's
// first vertex.  Checks the arguments and the tree (validate_flat) first and
// returns a vrhip_status value: 0, -1 (VRHIP_ERR_INVALID) or -4 (VRHIP_ERR_BVH).
int flat_trace_rays(const float* bvh, size_t n_bvh_f4, const float* verts, size_t n_slots, const float* origins,
                    const float* dirs, const float* tmax, uint32_t n_rays, uint32_t mode, RayHit* hits);

} // namespace vr
