// vr_atlas.hpp -- surface records without a ray: at caller-named points of
// the resident mesh (vrhip_surface_at) and at the texel centres of a W x H
// lightmap atlas of its UV unwrap (vrhip_atlas_surface).  The launchers, plain
// C++ for the host half; the kernels are vr_atlas.hip.  Both calls end in one
// fill kernel that runs fill_hit's mesh arm (vr_kernel.hpp) on (compact
// triangle, u, v), so a record is the one vrhip_trace_surface writes for a hit
// there; the atlas call first rasterises the uvs (include/vrhip.h has the
// definition: fp64 edge functions, canonical per edge, the smallest prim wins).
// No reference counterpart.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vr_params.hpp"
#include "vr_surface.hpp"

namespace vr {

constexpr uint32_t kAtlasMaxSide = 16384u;
constexpr uint64_t kAtlasMaxTexels = 1ull << 26;
constexpr uint32_t kAtlasMaxGutter = 64u;
constexpr uint32_t kAtlasNone = 0xffffffffu;      // no compact triangle: an unmapped prim, an uncovered texel

// The atlas intermediate, one 16-byte cell per texel: the winner's compact
// triangle in the low kAtlasIndexBits of word 0 with the gutter pass that
// reached the texel above them (0: covered by the triangle itself), then prim,
// u, v.  An uncovered texel's word 0 is kAtlasNone.
constexpr uint32_t kAtlasIndexBits = 25u;         // compact triangles < 2^24 + 127 (vr_devmesh.hpp leaf_code)
constexpr size_t kAtlasCellBytes = 16;
// scratch the atlas call needs: two cell planes (the winner words of the
// coverage pass live in the second) and the queue of large triangles
inline size_t atlas_scratch_bytes(uint64_t texels, uint32_t n_refs)
{
    return 2 * kAtlasCellBytes * (size_t)texels + sizeof(uint32_t) * ((size_t)n_refs + 4u);
}

// inv[prim] = the lowest compact triangle whose prim_id is prim, kAtlasNone
// where there is none: the inverse of MeshArrays::prim_id.  inv: u32[n_prims].
int launch_prim_inverse(const uint32_t* prim_id, uint32_t n_refs, uint32_t* inv, uint32_t n_prims, void* stream);

// vrhip_surface_at; every pointer is a device pointer
struct SurfaceAt {
    const uint32_t* prims;       // [n]
    const float* bary;           // float[2 n]: u, v, used as given
    uint32_t n;
    const uint32_t* inv;         // launch_prim_inverse's map
    uint32_t n_prims;
    SurfaceHit* hits;            // [n], 16-byte aligned
};
// p: the scene half of the launch parameters (vr_ctx.hpp scene_params) with
// the resident mesh in it.  Enqueues on `stream`; 0 or a hipError_t.  n > 0.
int launch_surface_at(const RenderParams& p, const SurfaceAt& q, void* stream);

// vrhip_atlas_surface
struct Atlas {
    uint32_t w, h, gutter;
    const uint32_t* prim_id;     // per compact triangle (vr_rayquery.hpp)
    void* scratch;               // atlas_scratch_bytes(w * h, p.n_tris), 16-byte aligned
    SurfaceHit* hits;            // [w h], 16-byte aligned
};
int launch_atlas_surface(const RenderParams& p, const Atlas& q, uint32_t cu_count, void* stream);

} // namespace vr
