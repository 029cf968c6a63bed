// vr_surface.hip -- the surface query (vr_surface.hpp): the dispatch over the
// feature sets, as launch_ray_radiance picks the radiance kernels', the
// generic set (kFeatAll: every feature tested against the launch's flags),
// which strict traversal and whatever the classes do not cover take, and the
// camera-ray kernel.
#include <hip/hip_runtime.h>

#include "vr_surface_dev.hpp"

namespace vr {

int launch_ray_surface(const RenderParams& p, const RaySurface& q, int stack, uint32_t cu_count, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint32_t cls = feature_class(p.flags & kFeatAll);
    if (cls == kClassCornellMesh) launch_surface_cornell_mesh(p, q, stack, cu_count, s);
    else if (cls == kClassHdriMesh) launch_surface_hdri_mesh(p, q, stack, cu_count, s);
    else if (cls == kClassCornellSphere || cls == kClassHdriSphere) launch_surface_sphere(p, q, cu_count, s);
    else launch_surface_stack<kFeatAll>(p, q, (p.flags & F_MESH) != 0u ? stack : 16, cu_count, s);
    return (int)hipGetLastError();
}

// One pixel per thread, row-major: camera_ray's origin and the operand of its
// normalize4, from the same table and in the same operation order, so that a
// query call that normalises the direction gets the pixel's camera ray.
__global__ void __launch_bounds__(kBlockThreads) camera_rays_kernel(const RenderParams p, float* origins, float* dirs)
{
    const uint64_t n = (uint64_t)p.W * p.H;
    const uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = (uint32_t)(i % p.W), y = (uint32_t)(i / p.W);
    const float sx = p.cam_sxy[x];
    const float sy = p.cam_sxy[p.W + y];
    const vr4 d = add4(add4(p.cam_d, mul4s(p.cx, sx)), mul4s(p.cy, sy));
    origins[3u * i] = p.cam_o.x; origins[3u * i + 1u] = p.cam_o.y; origins[3u * i + 2u] = p.cam_o.z;
    dirs[3u * i] = d.x; dirs[3u * i + 1u] = d.y; dirs[3u * i + 2u] = d.z;
}

int launch_camera_rays(const RenderParams& p, float* origins, float* dirs, void* stream)
{
    const uint64_t n = (uint64_t)p.W * p.H;
    const uint32_t blocks = (uint32_t)((n + kBlockThreads - 1u) / kBlockThreads);
    camera_rays_kernel<<<blocks, kBlockThreads, 0, (hipStream_t)stream>>>(p, origins, dirs);
    return (int)hipGetLastError();
}

} // namespace vr
