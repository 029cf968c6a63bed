// vr_refit.hpp -- refit of a device-built mesh (vr_refit.hip): new vertex
// positions under an unchanged tree, the boxes recomputed bottom-up over the
// emitted device layout (vr_mesh_layout.hpp DeviceMesh), and the tree's SAH
// cost.  No reference counterpart: the reference rebuilds on the host.
#pragma once
#include <cstddef>
#include <cstdint>

#include "vr_devmesh.hpp"

namespace vr {

// Everything below enqueues on `stream` and returns 0 or a hipError_t; all
// pointers are device pointers.

// level[i] = the depth of node i of the emitted node array (the root, node 0,
// is 0): a fill, then one launch per level, each writing the level below it.  `depth` is
// the tree's depth as DevBuildStatus counts it (root = 1).
int refit_levels(const vr4* bvh, uint32_t n_nodes, uint32_t depth, uint32_t* level, void* stream);

// Read-only: ORs DEVBVH_NONFINITE into st->flags when a position behind a
// compact slot of m is not finite (DEVBVH_BAD_INDEX when slot_vert itself is
// out of range).  st must be zero-filled on the stream before the call.
int refit_validate(const float* positions, uint32_t n_verts, const MeshArrays& m, DevBuildStatus* st, void* stream);

// m's verts, tri_e (and normals / tangents where given) gathered through
// slot_vert, then every child box of bvh and bvh16, one launch per level of
// node_level, deepest first; tpath, uvs and prim_id stay.  Only after
// refit_validate found nothing.
int refit_apply(const float* positions, const float* normals, const float* tangents, const MeshArrays& m,
                void* stream);

// SAH cost of the tree (1 per node, 1 per triangle) over the root's area, in
// fp64 with a fixed summation order over pairs (vr_devmesh.hpp Sum2), so the
// result is, in practice, flat_sah_cost's on the export bit for bit: partial holds two
// doubles per block of refit_cost_blocks(n_nodes), *cost the result (+inf for
// a root without area).
uint32_t refit_cost_blocks(uint32_t n_nodes);
int refit_sah_cost(const vr4* bvh, uint32_t n_nodes, double* partial, double* cost, void* stream);

} // namespace vr
