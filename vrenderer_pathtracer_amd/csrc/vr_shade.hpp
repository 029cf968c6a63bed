// vr_shade.hpp -- path-traced radiance from the caller's surface records
// (vrhip_shade_surface): the launcher of the query kernel, plain C++ for the
// host half.  The kernel (vr_shade_dev.hpp) is a fourth entry into the path
// tracer, next to vr_rayquery.hip, vr_radiance*.hip and vr_surface*.hip: the
// reference's trace (cuda/src/PathTracer.cu:597-770) with the hit of bounce 0
// read from a vrhip_surface_hit instead of intersected, bounces 1 to 3 the
// render's own.  No reference counterpart as a call.
// The kernel is instantiated per feature set in vr_shade.hip (the generic set
// and the dispatch) and vr_shade_{cornell_mesh,hdri_mesh,sphere}.hip, split as
// the radiance query's units are, so that they compile in parallel.
#pragma once
#include <stdint.h>

#include "vr_params.hpp"
#include "vr_surface.hpp"

namespace vr {

constexpr uint32_t kShadeMaxSamples = 4096;

// Records a wave takes at a time, one per lane (vr_shade_dev.hpp).
constexpr uint32_t kShadeSlice = 64;

// One launch of the query kernel; every pointer is a device pointer.
struct SurfaceShade {
    const SurfaceHit* hits;      // [n_hits], 16-byte aligned: kind as miss / hit, position, normal, tangent, color,
                                 // specular, emission and type are read
    const float* dirs;           // float[3 n_hits]: the incoming direction, normalised by the kernel (normalize4)
    const uint32_t* seeds;       // uint32[2 n_hits]: the seed pair each record's first path starts from
    uint32_t n_hits;
    uint32_t n_samples;          // paths per record, one after the other on the record's seed stream; 1..kShadeMaxSamples
    vr4* radiance;               // [n_hits], 16-byte aligned: rgb the mean over the paths, w 0
};

// p: the scene half of the launch parameters (vr_ctx.hpp scene_params); the
// camera, the tiling and the frame buffers are not read.  stack: 16, 24, 32 or
// 64 entries (tree depth + 1 at least; 16 without F_MESH in p.flags).
// Enqueues on `stream`; 0 or a hipError_t.  n_hits > 0.
int launch_surface_shade(const RenderParams& p, const SurfaceShade& q, int stack, uint32_t cu_count, void* stream);

} // namespace vr
