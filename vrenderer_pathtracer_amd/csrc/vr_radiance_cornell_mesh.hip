// vr_radiance_cornell_mesh.hip -- the radiance query kernels of feature class
// "Cornell box + mesh, any material features" (kClassCornellMesh), at every
// stack size.  One translation unit per class, so they compile in parallel.
#include "vr_radiance_dev.hpp"

namespace vr {

void launch_radiance_cornell_mesh(const RenderParams& p, const RayRadiance& q, int stack, uint32_t cu_count, hipStream_t s)
{
    launch_radiance_stack<kClassCornellMesh>(p, q, stack, cu_count, s);
}

} // namespace vr
