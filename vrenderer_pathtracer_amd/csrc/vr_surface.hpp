// vr_surface.hpp -- what the path tracer sees at the first hit of the
// caller's rays (vrhip_trace_surface), and the current camera's rays as a
// buffer (vrhip_camera_rays): the launchers, plain C++ for the host half.
// The kernel (vr_surface_dev.hpp) is a third entry into the path tracer, next
// to vr_rayquery.hip and vr_radiance*.hip: intersect_scene and fill_hit
// (vr_kernel.hpp; the reference's intersectScene, cuda/src/PathTracer.cu:
// 136-468) run once over a ray buffer, and the vHitData record every bounce
// of trace computes and consumes (cuda/include/PathTracer.cuh:17-53) is
// written out instead of shaded.  No reference counterpart as a call.
// The kernel is instantiated per feature set in vr_surface.hip (the generic
// set, the dispatch and the camera-ray kernel) and
// vr_surface_{cornell_mesh,hdri_mesh,sphere}.hip, split as the radiance
// query's units are, so that they compile in parallel.
#pragma once
#include <stdint.h>

#include "vr_params.hpp"

namespace vr {

// SurfaceHit::kind (VRHIP_SURF_*): the kernels' HitKind as it is (vr_kernel.hpp)
enum : uint32_t { kSurfNone = 0u, kSurfCornell = 1u, kSurfSmall = 2u, kSurfExample = 3u, kSurfMesh = 4u };

// vrhip_surface_hit: seven 16-byte rows
struct alignas(16) SurfaceHit {
    float t; uint32_t kind, prim, type;
    float position[3], bary_u;
    float normal[3], bary_v;
    float tangent[3], pad0;
    float color[3], tex_u;
    float specular[3], tex_v;
    float emission[3], pad1;
};

// One launch of the query kernel; every pointer is a device pointer.
struct RaySurface {
    const float* origins;        // float[3 n_rays], used as given
    const float* dirs;           // float[3 n_rays], normalised by the kernel (normalize4)
    uint32_t n_rays;
    const uint32_t* prim_id;     // per compact triangle, what SurfaceHit::prim reports (vr_rayquery.hpp); unread without F_MESH
    SurfaceHit* hits;            // [n_rays], 16-byte aligned
};

// p: the scene half of the launch parameters (vr_ctx.hpp scene_params); the
// camera, the tiling and the frame buffers are not read.  stack: 16, 24, 32 or
// 64 entries (tree depth + 1 at least; 16 without F_MESH in p.flags).
// Enqueues on `stream`; 0 or a hipError_t.  n_rays > 0.
int launch_ray_surface(const RenderParams& p, const RaySurface& q, int stack, uint32_t cu_count, void* stream);

// The camera half of p (vr_ctx.hpp camera_params: cam_o, cam_d, cx, cy, W, H,
// cam_sxy): per pixel, row-major, the origin and the operand of camera_ray's
// normalize4, (cam_d + cx * sx) + cy * sy.  origins, dirs: float[3 W H].
int launch_camera_rays(const RenderParams& p, float* origins, float* dirs, void* stream);

} // namespace vr
