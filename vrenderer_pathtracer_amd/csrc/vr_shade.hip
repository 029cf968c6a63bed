// vr_shade.hip -- radiance from the caller's surface records (vr_shade.hpp):
// the dispatch over the feature sets, as launch_ray_radiance picks the
// radiance query's, and the generic set (kFeatAll: every feature tested
// against the launch's flags), which strict traversal and whatever the
// classes do not cover take.
#include <hip/hip_runtime.h>

#include "vr_shade_dev.hpp"

namespace vr {

int launch_surface_shade(const RenderParams& p, const SurfaceShade& q, int stack, uint32_t cu_count, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint32_t cls = feature_class(p.flags & kFeatAll);
    if (cls == kClassCornellMesh) launch_shade_cornell_mesh(p, q, stack, cu_count, s);
    else if (cls == kClassHdriMesh) launch_shade_hdri_mesh(p, q, stack, cu_count, s);
    else if (cls == kClassCornellSphere || cls == kClassHdriSphere) launch_shade_sphere(p, q, cu_count, s);
    else launch_shade_stack<kFeatAll>(p, q, (p.flags & F_MESH) != 0u ? stack : 16, cu_count, s);
    return (int)hipGetLastError();
}

} // namespace vr
