// vr_radiance.hip -- the radiance query (vr_radiance.hpp): the dispatch over
// the feature sets, as launch_class picks the path kernels', and the generic
// set (kFeatAll: every feature tested against the launch's flags), which
// strict traversal and whatever the classes do not cover take.
#include <hip/hip_runtime.h>

#include "vr_radiance_dev.hpp"

namespace vr {

int launch_ray_radiance(const RenderParams& p, const RayRadiance& q, int stack, uint32_t cu_count, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint32_t cls = feature_class(p.flags & kFeatAll);
    if (cls == kClassCornellMesh) launch_radiance_cornell_mesh(p, q, stack, cu_count, s);
    else if (cls == kClassHdriMesh) launch_radiance_hdri_mesh(p, q, stack, cu_count, s);
    else if (cls == kClassCornellSphere || cls == kClassHdriSphere) launch_radiance_sphere(p, q, cu_count, s);
    else launch_radiance_stack<kFeatAll>(p, q, (p.flags & F_MESH) != 0u ? stack : 16, cu_count, s);
    return (int)hipGetLastError();
}

} // namespace vr
