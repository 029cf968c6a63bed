// vr_shade_cornell_mesh.hip -- the surface-record radiance kernels of feature
// class "Cornell box + mesh, any material features" (kClassCornellMesh), at
// every stack size.  One translation unit per class, so they compile in parallel.
#include "vr_shade_dev.hpp"

namespace vr {

void launch_shade_cornell_mesh(const RenderParams& p, const SurfaceShade& q, int stack, uint32_t cu_count, hipStream_t s)
{
    launch_shade_stack<kClassCornellMesh>(p, q, stack, cu_count, s);
}

} // namespace vr
