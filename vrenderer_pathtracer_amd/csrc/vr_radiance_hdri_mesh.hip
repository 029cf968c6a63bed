// vr_radiance_hdri_mesh.hip -- the radiance query kernels of feature class
// "HDRI environment + mesh, any material features" (kClassHdriMesh), at every
// stack size.  One translation unit per class, so they compile in parallel.
#include "vr_radiance_dev.hpp"

namespace vr {

void launch_radiance_hdri_mesh(const RenderParams& p, const RayRadiance& q, int stack, uint32_t cu_count, hipStream_t s)
{
    launch_radiance_stack<kClassHdriMesh>(p, q, stack, cu_count, s);
}

} // namespace vr
