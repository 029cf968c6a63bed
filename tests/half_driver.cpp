// Host driver for vr::half_directed (csrc/vr_devmesh.hpp), the device BVH
// builder's outward fp32 -> fp16 rounding: reads float bit patterns (hex, one
// per line) from stdin and prints "down up" (decimal half bit patterns) for
// each.  The function is the same source the kernels compile.
#include <cstdint>
#include <cstdio>

#include "vr_devmesh.hpp"

int main()
{
    unsigned int u;
    while (std::scanf("%x", &u) == 1)
        std::printf("%u %u\n", (unsigned)vr::half_directed((uint32_t)u, false), (unsigned)vr::half_directed((uint32_t)u, true));
    return 0;
}
