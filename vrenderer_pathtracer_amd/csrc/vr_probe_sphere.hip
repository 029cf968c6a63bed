// vr_probe_sphere.hip -- the probe kernels of the sphere feature classes
// (kClassCornellSphere, kClassHdriSphere): 16 stack entries and no mesh LDS,
// as render_kernel runs them.
#define VR_DK_HOISTED 1      // sphere-only kernels: the hoistable constant form (vr_math.hpp dk)
#include "vr_probe_dev.hpp"

namespace vr {

void launch_probe_sphere(const RenderParams& p, const ProbeSH& q, uint32_t cu_count, hipStream_t s)
{
    if ((p.flags & F_CORNELL) != 0u) launch_probe_one<16, kClassCornellSphere>(p, q, cu_count, s);
    else launch_probe_one<16, kClassHdriSphere>(p, q, cu_count, s);
}

} // namespace vr
