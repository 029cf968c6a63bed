// vrhip_mesh.cpp -- the resident triangle mesh (vr_ctx.hpp ResidentMesh): the
// host and the device upload, the refit, SAH costs, the export, and the calls
// on flattened trees that need no context (include/vrhip.h).  The queries
// along the caller's rays on the device: vrhip_query.cpp.
#include <cstring>

#include "vr_bvh.hpp"
#include "vr_ctx.hpp"
#include "vr_devbvh.hpp"
#include "vr_devsah.hpp"
#include "vr_mesh_layout.hpp"
#include "vr_rayquery.hpp"
#include "vr_refit.hpp"

namespace {

// One member's share of vrhip_upload_mesh_flat: the prepared arrays into a
// fresh mesh, swapped in once every copy has arrived.  After it the refit
// arrays are absent and prim_id holds flat slots.
int one_upload_mesh(vrhip_ctx* c, const vr::DeviceMesh& dm, uint32_t depth, uint32_t nodes, size_t n_bvh_f4,
                    size_t n_slots)
{
    int rc = set_device(c); if (rc) return rc;
    quiesce(c);
    ResidentMesh m;
    // a mesh without a triangle carries one padding entry per array: within the 16 bytes every array has
    const uint32_t n_nodes = (uint32_t)(dm.nodes.size() / 4), n_refs = (uint32_t)(dm.tris.size() / 3);
    if ((rc = m.alloc(n_nodes, n_refs, false))) return rc;
    auto put = [&](void* dst, const auto& v) {
        return v.empty() ? hipSuccess
                         : hipMemcpyAsync(dst, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, c->stream);
    };
    HIP_TRY(put(m.a.bvh, dm.nodes));
    HIP_TRY(put(m.a.bvh16, dm.nodes16));
    HIP_TRY(put(m.a.verts, dm.tris));
    HIP_TRY(put(m.a.tri_e, dm.tri_e));
    HIP_TRY(put(m.a.tpath, dm.tpath));
    HIP_TRY(put(m.a.normals, dm.normals));
    HIP_TRY(put(m.a.tangents, dm.tangents));
    HIP_TRY(put(m.a.uvs, dm.uvs));
    HIP_TRY(put(m.a.prim_id, dm.prim_id));
    HIP_TRY(hipStreamSynchronize(c->stream));
    m.a.n_nodes = n_nodes; m.a.n_refs = n_refs; m.a.depth = depth;
    m.n_bvh = n_bvh_f4; m.n_slots = n_slots; m.bvh_nodes = nodes;
    m.n_prims = (uint32_t)n_slots;                // prim_id holds flat slots
    c->mesh.swap(m);
    return VRHIP_OK;
}

// What a build and a refit do around their kernels: the status record zeroed,
// `launch` run (0 or a hipError_t), the record read back into st and the
// stream waited for.  A flag in `callers` is an error of the caller's
// arguments, any other an internal one.
template <typename F>
int run_with_status(vrhip_ctx* c, vr::DevBuildStatus* d_st, const char* what, uint32_t callers,
                    vr::DevBuildStatus& st, F&& launch)
{
    HIP_TRY(hipMemsetAsync(d_st, 0, sizeof(vr::DevBuildStatus), c->stream));
    const int e = launch();
    if (e) return fail(VRHIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipMemcpyAsync(&st, d_st, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t f = st.flags & callers;
    if (f & vr::DEVBVH_BAD_INDEX) return fail(VRHIP_ERR_INVALID, "a triangle index is >= n_verts");
    if (f & vr::DEVBVH_NONFINITE) return fail(VRHIP_ERR_INVALID, "a referenced vertex position is not finite");
    if (f & vr::DEVBVH_BIG_LEAF) return fail(VRHIP_ERR_BVH, "leaf with >= 128 triangles");
    if (st.flags) return fail(VRHIP_ERR_BVH, std::string(what) + ": internal inconsistency");
    return VRHIP_OK;
}

// The five arrays of a flattened mesh into the caller's, or only the sizes
// they need when one of them is null.
int flat_out(const vr::FlatMesh& m, float* bvh, size_t* n_bvh_f4, float* verts, float* normals, float* tangents,
             float* uvs, size_t* n_slots)
{
    if (bvh && verts && normals && tangents && uvs) {
        if (*n_bvh_f4 < m.bvh.size() || *n_slots < m.verts.size()) return fail(VRHIP_ERR_INVALID, "output arrays too small");
        std::memcpy(bvh, m.bvh.data(), m.bvh.size() * 16);
        std::memcpy(verts, m.verts.data(), m.verts.size() * 16);
        std::memcpy(normals, m.normals.data(), m.normals.size() * 16);
        std::memcpy(tangents, m.tangents.data(), m.tangents.size() * 16);
        std::memcpy(uvs, m.uvs.data(), m.uvs.size() * 8);
    }
    *n_bvh_f4 = m.bvh.size();
    *n_slots = m.verts.size();
    return VRHIP_OK;
}

} // namespace

// The tree is validated and laid out for the device once; every member of a
// multi-device context then uploads the same arrays.  A member that fails
// ends the call: the members before it hold the new mesh, it and the members
// after it the one they had.
int vrhip_upload_mesh_flat(vrhip_ctx* c, const float* bvh, size_t n_bvh_f4, const float* verts, const float* normals,
                           const float* tangents, const float* uvs, size_t n_slots)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (!bvh || !verts || !normals || !tangents || !uvs) return fail(VRHIP_ERR_INVALID, "null mesh array");
    uint32_t depth = 0, nodes = 0;
    int v = vr::validate_flat(bvh, n_bvh_f4, verts, n_slots, &depth, &nodes);
    if (v != 0) return fail(VRHIP_ERR_BVH, "flattened BVH failed validation (code " + std::to_string(v) + ")");
    if (depth > 62) return fail(VRHIP_ERR_BVH, "BVH deeper than 62 levels");
    vr::DeviceMesh dm;
    std::string why;
    if (!vr::to_device_layout(bvh, n_bvh_f4, (const vr4*)verts, (const vr4*)normals, (const vr4*)tangents,
                              (const vr2*)uvs, dm, why))
        return fail(VRHIP_ERR_BVH, why);
    const std::vector<vrhip_ctx*> alone{ c };
    for (vrhip_ctx* m : c->group.empty() ? alone : c->group) {
        const int rc = one_upload_mesh(m, dm, depth, nodes, n_bvh_f4, n_slots);
        if (rc != VRHIP_OK) return rc;
    }
    return VRHIP_OK;
}

int vrhip_upload_mesh_indexed(vrhip_ctx* c, const float* positions, const float* normals, const float* tangents,
                              const float* uvs, uint32_t n_verts, const uint32_t* tris, uint32_t n_tris,
                              uint32_t max_leaf_tris)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    vr::FlatMesh m;
    if (vr::build_flat(positions, normals, tangents, uvs, n_verts, tris, n_tris, max_leaf_tris, m) != 0)
        return fail(VRHIP_ERR_INVALID, "BVH build failed (empty mesh or bad indices)");
    return vrhip_upload_mesh_flat(c, (const float*)m.bvh.data(), m.bvh.size(), (const float*)m.verts.data(),
                                  (const float*)m.normals.data(), (const float*)m.tangents.data(),
                                  (const float*)m.uvs.data(), m.verts.size());
}

int vrhip_upload_mesh_device(vrhip_ctx* c, const float* d_positions, const float* d_normals, const float* d_tangents,
                             const float* d_uvs, uint32_t n_verts, const uint32_t* d_tris, uint32_t n_tris,
                             uint32_t max_leaf_tris)
{
    return vrhip_upload_mesh_device_ex(c, d_positions, d_normals, d_tangents, d_uvs, n_verts, d_tris, n_tris,
                                       max_leaf_tris, VRHIP_DEVBVH_MORTON);
}

// The device builders' entry point: the mesh is built from device-resident
// triangles into a fresh ResidentMesh, as the host upload fills one.
// builder: the Morton tree of vr_devbvh.hip (its shape is closed-form, so the
// arrays are sized exactly) or the host's binned-SAH tree of vr_devsah.hip
// (sized for the worst case of n_refs - 1 nodes; the build reports its shape).
int vrhip_upload_mesh_device_ex(vrhip_ctx* c, const float* d_positions, const float* d_normals,
                                const float* d_tangents, const float* d_uvs, uint32_t n_verts, const uint32_t* d_tris,
                                uint32_t n_tris, uint32_t max_leaf_tris, uint32_t builder)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (!d_positions || !d_tris || n_tris == 0 || n_verts == 0) return fail(VRHIP_ERR_INVALID, "null or empty mesh arrays");
    if (n_tris >= (1u << (31 - vr::kLeafCountBits))) return fail(VRHIP_ERR_INVALID, "more than 16M triangles");
    if (max_leaf_tris >= (1u << vr::kLeafCountBits)) return fail(VRHIP_ERR_INVALID, "max_leaf_tris above 127");
    if (builder != VRHIP_DEVBVH_MORTON && builder != VRHIP_DEVBVH_SAH) return fail(VRHIP_ERR_INVALID, "unknown device builder");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_upload_mesh_device");
    const bool sah = builder == VRHIP_DEVBVH_SAH;
    const uint32_t max_leaf = max_leaf_tris ? max_leaf_tris : 2u;
    vr::DevBuildShape sh = vr::devbvh_shape(n_tris, max_leaf);
    if (sah) sh.nodes = sh.n_refs - 1u;           // the worst case: one triangle per leaf
    int rc = set_device(c); if (rc) return rc;
    quiesce(c);
    ResidentMesh m;
    if ((rc = m.alloc(sh.nodes, sh.n_refs, true))) return rc;
    void* scratch = nullptr;
    vr::DevBuildStatus st{};
    rc = run_with_status(c, m.status, "device BVH build",
                         vr::DEVBVH_BAD_INDEX | vr::DEVBVH_NONFINITE | vr::DEVBVH_BIG_LEAF, st, [&] {
                             return (sah ? vr::devsah_build : vr::devbvh_build)(d_positions, d_normals, d_tangents, d_uvs,
                                                                               n_verts, d_tris, n_tris, max_leaf, m.a,
                                                                               m.status, &scratch, c->stream);
                         });
    const dev_ptr<void> arena(scratch);           // the builder's scratch: the stream has finished with it
    if (rc) return rc;
    if (sah ? (st.nodes == 0 || st.nodes > sh.nodes || st.leaves != st.nodes + 1u || st.depth == 0 ||
               st.depth > vr::kMaxBuildDepth)
            : (st.depth != sh.depth || st.nodes != sh.nodes || st.leaves != sh.leaves || st.depth > 62))
        return fail(VRHIP_ERR_BVH, "device BVH build: the tree is not the shape its size gives");
    m.a.n_nodes = st.nodes; m.a.n_refs = sh.n_refs; m.a.depth = st.depth;
    m.n_bvh = 4 * (size_t)st.nodes; m.n_slots = st.slots; m.bvh_nodes = st.nodes;
    m.refit_verts = n_verts;
    m.n_prims = n_tris;
    c->mesh.swap(m);
    return VRHIP_OK;
}

size_t vrhip_device_sah_scratch_bytes(uint32_t n_tris) { return vr::devsah_arena_bytes(n_tris); }

// New vertex positions under the resident tree (vr_refit.hip): a read-only
// validation pass and its read-back first, so a refused call writes nothing.
int vrhip_refit_mesh_device(vrhip_ctx* c, const float* d_positions, const float* d_normals, const float* d_tangents,
                            uint32_t n_verts)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (!d_positions) return fail(VRHIP_ERR_INVALID, "null positions");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_refit_mesh_device");
    const ResidentMesh& m = c->mesh;
    if (!m.loaded()) return fail(VRHIP_ERR_INVALID, "no mesh loaded");
    if (!m.a.slot_vert || !m.a.node_level || !m.status)
        return fail(VRHIP_ERR_INVALID, "the resident mesh was not built on the device (it keeps no index data)");
    if (n_verts != m.refit_verts)
        return fail(VRHIP_ERR_INVALID, "n_verts is " + std::to_string(n_verts) + ", the upload's was " +
                                           std::to_string(m.refit_verts));
    int rc = set_device(c); if (rc) return rc;
    quiesce(c);
    vr::DevBuildStatus st{};
    rc = run_with_status(c, m.status, "mesh refit", vr::DEVBVH_NONFINITE, st,
                         [&] { return vr::refit_validate(d_positions, n_verts, m.a, m.status, c->stream); });
    if (rc) return rc;
    const int e = vr::refit_apply(d_positions, d_normals, d_tangents, m.a, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("mesh refit: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VRHIP_OK;
}

int vrhip_bvh_sah_cost(vrhip_ctx* c, double* cost)
{
    if (!c || !cost) return fail(VRHIP_ERR_INVALID, "null argument");
    if (!c->mesh.loaded()) return fail(VRHIP_ERR_INVALID, "no mesh loaded");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    const vr::MeshArrays& a = c->mesh.a;
    const uint32_t nb = vr::refit_cost_blocks(a.n_nodes);
    dev_ptr<double> buf;                          // the block partials (a pair each), then the result
    HIP_TRY(dev_alloc(buf, (2 * (size_t)nb + 1) * sizeof(double)));
    const int e = vr::refit_sah_cost(a.bvh, a.n_nodes, buf.get(), buf.get() + 2 * (size_t)nb, c->stream);
    hipError_t he = e ? (hipError_t)e
                      : hipMemcpyAsync(cost, buf.get() + 2 * (size_t)nb, sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    if (he != hipSuccess) return fail(VRHIP_ERR_HIP, std::string("SAH cost: ") + hipGetErrorString(he));
    return svc_verify(c);
}

int vrhip_flat_sah_cost(const float* bvh, size_t n_bvh_f4, const float* verts, size_t n_slots, double* cost)
{
    if (!cost) return fail(VRHIP_ERR_INVALID, "cost is NULL");
    const int v = vr::validate_flat(bvh, n_bvh_f4, verts, n_slots, nullptr, nullptr);
    if (v != 0) return fail(VRHIP_ERR_BVH, "validation failed (code " + std::to_string(v) + ")");
    *cost = vr::flat_sah_cost(bvh, verts);
    return VRHIP_OK;
}

int vrhip_flat_trace_rays(const float* bvh, size_t n_bvh_f4, const float* verts, size_t n_slots, const float* origins,
                          const float* dirs, const float* tmax, uint32_t n_rays, uint32_t mode, vrhip_ray_hit* hits)
{
    const int rc = vr::flat_trace_rays(bvh, n_bvh_f4, verts, n_slots, origins, dirs, tmax, n_rays, mode,
                                       (vr::RayHit*)hits);
    if (rc == VRHIP_ERR_BVH) return fail(VRHIP_ERR_BVH, "flattened BVH failed validation");
    if (rc != VRHIP_OK) return fail(VRHIP_ERR_INVALID, "null array or unknown ray query mode");
    return VRHIP_OK;
}

// The resident mesh back in the reference layout: the LIFO flatten of
// vr::build_flat over the device tree, so the result does not depend on the
// device's node order.
int vrhip_export_mesh_flat(vrhip_ctx* c, float* bvh, size_t* n_bvh_f4, float* verts, float* normals, float* tangents,
                           float* uvs, size_t* n_slots)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (!n_bvh_f4 || !n_slots) return fail(VRHIP_ERR_INVALID, "size outputs are required");
    if (!c->mesh.loaded()) return fail(VRHIP_ERR_INVALID, "no mesh loaded");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    const vr::MeshArrays& a = c->mesh.a;
    const size_t nv = 3 * (size_t)a.n_refs;
    std::vector<vr4> dn(4 * (size_t)a.n_nodes), dnrm(nv), dtan(nv);
    std::vector<vr3> dv(nv);
    std::vector<vr2> duv(nv);
    HIP_TRY(hipMemcpyAsync(dn.data(), a.bvh, dn.size() * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dv.data(), a.verts, nv * sizeof(vr3), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dnrm.data(), a.normals, nv * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dtan.data(), a.tangents, nv * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(duv.data(), a.uvs, nv * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = svc_verify(c)) != VRHIP_OK) return rc;
    vr::FlatMesh flat;
    if (!vr::device_to_flat(dn, dv, dnrm, dtan, duv, flat)) return fail(VRHIP_ERR_BVH, "resident tree is malformed");
    return flat_out(flat, bvh, n_bvh_f4, verts, normals, tangents, uvs, n_slots);
}

int vrhip_bvh_info(vrhip_ctx* c, uint32_t* depth, uint32_t* n_nodes, uint32_t* n_slots)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (depth) *depth = c->mesh.a.depth;
    if (n_nodes) *n_nodes = c->mesh.bvh_nodes;
    if (n_slots) *n_slots = (uint32_t)c->mesh.n_slots;
    return VRHIP_OK;
}

int vrhip_build_flat(const float* positions, const float* normals, const float* tangents, const float* uvs,
                     uint32_t n_verts, const uint32_t* tris, uint32_t n_tris, uint32_t max_leaf_tris,
                     float* bvh_out, size_t* n_bvh_f4, float* verts_out, float* normals_out,
                     float* tangents_out, float* uvs_out, size_t* n_slots)
{
    if (!n_bvh_f4 || !n_slots) return fail(VRHIP_ERR_INVALID, "size outputs are required");
    vr::FlatMesh m;
    if (vr::build_flat(positions, normals, tangents, uvs, n_verts, tris, n_tris, max_leaf_tris, m) != 0)
        return fail(VRHIP_ERR_INVALID, "BVH build failed (empty mesh or bad indices)");
    return flat_out(m, bvh_out, n_bvh_f4, verts_out, normals_out, tangents_out, uvs_out, n_slots);
}

int vrhip_validate_flat(const float* bvh, size_t n_bvh_f4, const float* verts, size_t n_slots,
                        uint32_t* depth, uint32_t* n_nodes)
{
    int v = vr::validate_flat(bvh, n_bvh_f4, verts, n_slots, depth, n_nodes);
    if (v != 0) return fail(VRHIP_ERR_BVH, "validation failed (code " + std::to_string(v) + ")");
    return VRHIP_OK;
}
