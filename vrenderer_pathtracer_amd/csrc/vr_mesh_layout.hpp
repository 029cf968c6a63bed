// vr_mesh_layout.hpp -- the flattened reference tree (vr_bvh.hpp FlatMesh) to
// the device mesh layout and back (vr_mesh_layout.cpp).  Host C++ only: no
// HIP, no context, so the sanitizer driver (tests/sanitize_driver.cpp) compiles it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "vr_bvh.hpp"
#include "vr_params.hpp"

namespace vr {

// Device mesh layout (see vr_kernel.hip): the reference nodes with leaf
// children re-encoded as ~((first_tri << 7) | count) into compact per-triangle
// arrays (3 slots per triangle, terminator slots dropped).  Built from the
// reference flattening (src/vRendererCuda.cpp:204-279) so the triangles a
// leaf tests, and their order, are exactly the reference's.
struct DeviceMesh {
    std::vector<vr4> nodes, normals, tangents;
    std::vector<vr4> nodes16;        // 2 x 16 B per node: conservative fp16 boxes + child indices
    std::vector<vr3> tris;           // packed 12 B vertices (vertex .w never reaches a result)
    std::vector<vr3> tri_e;          // per triangle v0, v1 - v0, v2 - v0 (fp32, the kernel's own subtractions)
    std::vector<unsigned long long> tpath;   // per triangle: leaf path from the root under a leading 1 bit
    std::vector<vr2> uvs;
    std::vector<uint32_t> prim_id;   // per triangle: the flat slot of its first vertex (what a ray query reports)
};

// The arrays must have passed validate_flat.  false: refused, with the reason in `why`.
bool to_device_layout(const float* bvh, size_t n_bvh_f4, const vr4* verts, const vr4* normals,
                      const vr4* tangents, const vr2* uvs, DeviceMesh& dm, std::string& why);

// The device arrays (nodes: 4 rows per node; verts, normals, tangents, uvs: 3
// entries per compact triangle) back in the reference layout: the LIFO flatten
// of build_flat over the device tree, so the result does not depend on the
// device's node order.  false: the tree is malformed.
bool device_to_flat(const std::vector<vr4>& nodes, const std::vector<vr3>& verts, const std::vector<vr4>& normals,
                    const std::vector<vr4>& tangents, const std::vector<vr2>& uvs, FlatMesh& out);

} // namespace vr
