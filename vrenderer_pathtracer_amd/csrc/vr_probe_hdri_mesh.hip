// vr_probe_hdri_mesh.hip -- the probe kernels of feature class "HDRI + mesh,
// any material features" (kClassHdriMesh), at every stack size.  One
// translation unit per class, so they compile in parallel.
#include "vr_probe_dev.hpp"

namespace vr {

void launch_probe_hdri_mesh(const RenderParams& p, const ProbeSH& q, int stack, uint32_t cu_count, hipStream_t s)
{
    launch_probe_stack<kClassHdriMesh>(p, q, stack, cu_count, s);
}

} // namespace vr
