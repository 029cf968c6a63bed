// vr_surface_hdri_mesh.hip -- the surface query kernels of feature class
// "HDRI + mesh, any material features" (kClassHdriMesh), at every stack size.
// One translation unit per class, so they compile in parallel.
#include "vr_surface_dev.hpp"

namespace vr {

void launch_surface_hdri_mesh(const RenderParams& p, const RaySurface& q, int stack, uint32_t cu_count, hipStream_t s)
{
    launch_surface_stack<kClassHdriMesh>(p, q, stack, cu_count, s);
}

} // namespace vr
