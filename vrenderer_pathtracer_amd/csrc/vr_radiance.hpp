// vr_radiance.hpp -- path-traced radiance along the caller's rays
// (vrhip_trace_radiance): the launcher of the query kernel, plain C++ for the
// host half.  The kernel (vr_radiance_dev.hpp) is a second entry into the path
// tracer, as vr_rayquery.hip is into traverse_mesh: render_kernel's own
// sequence per pixel (intersect_scene once, the shared escape of HDRI scenes,
// trace<> per path, the sum in path order; vr_kernel.hpp, the reference's
// render and trace, cuda/src/PathTracer.cu:597-770, :791-868) run over a ray
// buffer instead of camera_ray.  No reference counterpart as a call: the
// reference traces its one camera only.
// The kernel is instantiated per feature set in vr_radiance.hip (the generic
// set and the dispatch) and vr_radiance_{cornell_mesh,hdri_mesh,sphere}.hip,
// split as the path kernels' vr_cls_*.hip are, so that they compile in parallel.
#pragma once
#include <stdint.h>

#include "vr_params.hpp"

namespace vr {

constexpr uint32_t kRadianceMaxSamples = 4096;

// One launch of the query kernel; every pointer is a device pointer.
struct RayRadiance {
    const float* origins;        // float[3 n_rays], used as given
    const float* dirs;           // float[3 n_rays], normalised by the kernel (normalize4)
    const uint32_t* seeds;       // uint32[2 n_rays]: the seed pair each ray's first path starts from
    uint32_t n_rays;
    uint32_t n_samples;          // paths per ray, one after the other on the ray's seed stream; 1..kRadianceMaxSamples
    vr4* radiance;               // [n_rays], 16-byte aligned: rgb the mean over the paths, w the last path's depth term
};

// p: the scene half of the launch parameters (vr_ctx.hpp scene_params); the
// camera, the tiling and the frame buffers are not read.  stack: 16, 24, 32 or
// 64 entries (tree depth + 1 at least; 16 without F_MESH in p.flags).
// Enqueues on `stream`; 0 or a hipError_t.  n_rays > 0.
int launch_ray_radiance(const RenderParams& p, const RayRadiance& q, int stack, uint32_t cu_count, void* stream);

} // namespace vr
