// vrhip_scene.cpp -- the context and what it holds: create / destroy, stream,
// camera and flags, mesh / environment / texture / BRDF uploads, asset
// loaders, GL presentation, read-backs and info getters (include/vrhip.h).
#include <hip/hip_runtime.h>
#include <hip/hip_gl_interop.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "vr_bvh.hpp"
#include "vr_ctx.hpp"
#include "vr_devbvh.hpp"
#include "vr_devsah.hpp"
#include "vr_exr.hpp"
#include "vr_merl.hpp"
#include "vr_mesh_layout.hpp"
#include "vr_rayquery.hpp"
#include "vr_refit.hpp"

namespace {

thread_local std::string g_last_error;

// Reference default camera fov: Camera::getFovScale (src/Camera.cpp:4,119-123)
float default_fov_scale()
{
    const float kDegInRad = (float)(M_PI / 180.f);
    const float fovRad = 75.f * kDegInRad;
    return std::tan(fovRad / 2.f);
}

int clear_accum(vrhip_ctx* c)
{
    int rc = svc_close(c);                        // the open session's results come first
    if (rc != VRHIP_OK) return rc;
    ++c->stream_epoch;
    c->frame = 1;
    HIP_TRY(hipMemsetAsync(c->accum, 0, sizeof(vr4) * (size_t)c->W * c->H, c->stream));
    return VRHIP_OK;
}

template <typename T>
int upload(vrhip_ctx* c, T*& dst, const void* src, size_t bytes)
{
    quiesce(c);
    dfree(dst);
    HIP_TRY(hipMalloc((void**)&dst, bytes ? bytes : 16));
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return VRHIP_OK;
}

} // namespace

int fail(int code, const std::string& msg) { g_last_error = msg; return code; }

const char* vrhip_last_error(void) { return g_last_error.c_str(); }
int vrhip_abi_version(void) { return VRHIP_ABI_VERSION; }

// SHA-256 of the sources, include/vrhip.h and the compile flags this library
// was built from, tagged so build.py can read it from the file without
// loading it (vrenderer_pathtracer_amd/build.py passes it in)
#ifndef VRHIP_BUILD_ID
#define VRHIP_BUILD_ID "vrhip-build-id:unknown"
#endif
const char* vrhip_build_id(void)
{
    static const char id[] = VRHIP_BUILD_ID;
    static const char tag[] = "vrhip-build-id:";
    return std::strncmp(id, tag, sizeof(tag) - 1) == 0 ? id + sizeof(tag) - 1 : id;
}

int vrhip_device_count(int* count)
{
    if (!count) return fail(VRHIP_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(VRHIP_ERR_NO_DEVICE, hipGetErrorString(e)); }
    *count = n;
    return VRHIP_OK;
}

int vrhip_create(int device, uint32_t width, uint32_t height, vrhip_ctx** out)
{
    if (!out || width == 0 || height == 0 || width > 65535 || height > 65535)
        return fail(VRHIP_ERR_INVALID, "bad create arguments (1..65535 pixels per side)");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(VRHIP_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= n) return fail(VRHIP_ERR_INVALID, "device index out of range");
    vrhip_ctx* c = new vrhip_ctx();
    c->device = device;
    c->W = width; c->H = height;
    c->fov_scale = default_fov_scale();
    if (const char* e = std::getenv("VRHIP_COST_ORDER")) c->cost_order = std::atoi(e) != 0;
    if (const char* e = std::getenv("VRHIP_KERNEL_TIMING")) c->kernel_timing = std::atoi(e) != 0;
    if (const char* e = std::getenv("VRHIP_GRAPH")) c->use_graph = std::atoi(e) != 0;
    if (const char* e = std::getenv("VRHIP_SYNC_FLAG")) c->sync_flag_mode = std::atoi(e) != 0 ? 1 : 0;
    if (const char* e = std::getenv("VRHIP_SERVICE")) c->service = std::max(-1, std::min(1, std::atoi(e)));
    int rc;
    if ((rc = set_device(c)) != VRHIP_OK) { delete c; return rc; }
    auto cleanup = [&](int code) { vrhip_destroy(c); return code; };
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess)
        return cleanup(fail(VRHIP_ERR_HIP, "hipStreamCreate failed"));
    c->stream = c->own_stream;
    for (auto& l : c->lane) {
        if (hipStreamCreateWithFlags(&l.s, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&l.done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&l.finished, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&l.ordered[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&l.ordered[1], hipEventDisableTiming) != hipSuccess)
            return cleanup(fail(VRHIP_ERR_HIP, "path stream setup failed"));
    }
    if (hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess)
        return cleanup(fail(VRHIP_ERR_HIP, "hipEventCreate failed"));
    if (hipMalloc((void**)&c->tone_t, 256 * sizeof(float)) != hipSuccess ||
        vr::launch_tone_table(c->tone_t, c->stream) != 0)
        return cleanup(fail(VRHIP_ERR_HIP, "tonemap table setup failed"));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        c->cu_count = (uint32_t)cus;
    const size_t npx = (size_t)width * height;
    if (hipMalloc((void**)&c->accum, sizeof(vr4) * npx) != hipSuccess ||
        hipMalloc((void**)&c->rgba, 4 * npx) != hipSuccess ||
        hipMalloc((void**)&c->depth, 4 * npx) != hipSuccess)
        return cleanup(fail(VRHIP_ERR_NOMEM, "hipMalloc of frame buffers failed"));
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess)
        return cleanup(fail(VRHIP_ERR_HIP, "hipEventCreate failed"));
    {
        // the camera ray's screen offsets (PathTracer.cu:842-843), evaluated
        // in double as there, once per column and row: the kernels index
        // them instead of dividing in f64 per ray
        std::vector<float> sxy((size_t)width + height);
        for (uint32_t x = 0; x < width; ++x) sxy[x] = (float)((0.25 + (double)x) / (double)width - 0.5);
        for (uint32_t y = 0; y < height; ++y) sxy[(size_t)width + y] = (float)((0.25 + (double)y) / (double)height - 0.5);
        if (hipMalloc((void**)&c->cam_sxy, sizeof(float) * sxy.size()) != hipSuccess)
            return cleanup(fail(VRHIP_ERR_NOMEM, "hipMalloc of the camera table failed"));
        if (hipMemcpy(c->cam_sxy, sxy.data(), sizeof(float) * sxy.size(), hipMemcpyHostToDevice) != hipSuccess)
            return cleanup(fail(VRHIP_ERR_HIP, "camera table upload failed"));
    }
    if (hipMemsetAsync(c->rgba, 0, 4 * npx, c->stream) != hipSuccess ||
        hipMemsetAsync(c->depth, 0, 4 * npx, c->stream) != hipSuccess)
        return cleanup(fail(VRHIP_ERR_HIP, "hipMemset failed"));
    if ((rc = clear_accum(c)) != VRHIP_OK) return cleanup(rc);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return cleanup(fail(VRHIP_ERR_HIP, "sync failed"));
    *out = c;
    return VRHIP_OK;
}

int vrhip_destroy(vrhip_ctx* c)
{
    if (!c) return VRHIP_OK;
    if (!c->group.empty()) {                          // a multi-device context: every member, the lead last
        std::vector<vrhip_ctx*> ms;
        ms.swap(c->group);
        for (vrhip_ctx* m : ms) { (void)hipSetDevice(m->device); (void)svc_close(m); if (m->stream) (void)hipStreamSynchronize(m->stream); }
        for (size_t i = ms.size(); i-- > 1;) vrhip_destroy(ms[i]);
    }
    (void)hipSetDevice(c->device);
    (void)svc_close(c);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    quiesce(c);
    dfree(c->accum); dfree(c->rgba); dfree(c->depth); dfree(c->cam_sxy);
    dfree(c->bvh); dfree(c->bvh16); dfree(c->verts); dfree(c->tri_e); dfree(c->tpath); dfree(c->normals); dfree(c->tangents); dfree(c->uvs);
    dfree(c->slot_vert); dfree(c->node_level); dfree(c->refit_status); dfree(c->prim_id);
    dfree(c->hdr); dfree(c->tex[0]); dfree(c->tex[1]); dfree(c->tex[2]); dfree(c->brdf);
    for (int i = 0; i < 2; ++i)
        if (c->gl_res[i]) (void)hipGraphicsUnregisterResource(c->gl_res[i]);
    dfree(c->counters); dfree(c->tone_t);
    if (c->comm) (void)ncclCommDestroy(c->comm);
    dfree(c->comm_send); dfree(c->comm_recv);
    for (auto& l : c->lane) {
        dfree(l.paths); dfree(l.prim); dfree(l.chunk_ctr); dfree(l.px_list);
        for (int i = 0; i < 2; ++i) { dfree(l.sub_cost[i]); dfree(l.sub_order[i]); }
        if (l.done) (void)hipEventDestroy(l.done);
        for (int i = 0; i < 2; ++i)
            if (l.ordered[i]) (void)hipEventDestroy(l.ordered[i]);
        if (l.finished) (void)hipEventDestroy(l.finished);
        if (l.s) (void)hipStreamDestroy(l.s);
    }
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (auto& pr : c->kev_pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    svc_free(c);
    for (hipEvent_t e : c->kev_free) (void)hipEventDestroy(e);
    if (c->kev_origin) (void)hipEventDestroy(c->kev_origin);
    for (auto& G : c->fgraph) {
        if (G.x) (void)hipGraphExecDestroy(G.x);
        if (G.g) (void)hipGraphDestroy(G.g);
    }
    if (c->sync_flag) (void)hipHostFree(c->sync_flag);
    dfree(c->sync_ctr);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return VRHIP_OK;
}

int vrhip_set_stream(vrhip_ctx* c, void* s)
{
    if (c && !c->group.empty()) return refuse_multi(c, "vrhip_set_stream");
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    c->stream_shared = true;            // the caller may queue its own work on it: vrhip_sync waits for the stream
    // work queued on the old stream (finish passes) must not reorder with the new one
    if (c->stream && hipSetDevice(c->device) == hipSuccess) {
        (void)svc_close(c);
        (void)hipStreamSynchronize(c->stream);
    }
    quiesce(c);
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return VRHIP_OK;
}

void* vrhip_get_stream(vrhip_ctx* c)
{
    if (!c) return nullptr;
    c->stream_shared = true;            // the caller may queue its own work on it: vrhip_sync waits for the stream
    c->flag_armed = 0;
    return (void*)c->stream;
}

int one_set_camera(vrhip_ctx* c, const float origin[3], const float dir[3], const float up[3],
                     const float right[3], float fov_scale)
{
    if (!c || !origin || !dir || !up || !right) return fail(VRHIP_ERR_INVALID, "bad camera arguments");
    std::memcpy(c->cam_o, origin, 12); std::memcpy(c->cam_d, dir, 12);
    std::memcpy(c->cam_up, up, 12); std::memcpy(c->cam_right, right, 12);
    c->fov_scale = fov_scale;
    int rc = set_device(c); if (rc) return rc;
    return clear_accum(c);
}

int one_clear(vrhip_ctx* c)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    int rc = set_device(c); if (rc) return rc;
    return clear_accum(c);
}

int one_set_fresnel(vrhip_ctx* c, float coef, float power)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    c->fresnel_coef = coef; c->fresnel_pow = power;
    return VRHIP_OK;
}

int one_use_cornell_box(vrhip_ctx* c, int e) { if (!c) return fail(VRHIP_ERR_INVALID, "null ctx"); c->cornell = e != 0; return VRHIP_OK; }
int one_use_example_sphere(vrhip_ctx* c, int e) { if (!c) return fail(VRHIP_ERR_INVALID, "null ctx"); c->example = e != 0; return VRHIP_OK; }
int one_set_strict_traversal(vrhip_ctx* c, int e) { if (!c) return fail(VRHIP_ERR_INVALID, "null ctx"); c->strict = e != 0; return VRHIP_OK; }
int one_use_brdf(vrhip_ctx* c, int e) { if (!c) return fail(VRHIP_ERR_INVALID, "null ctx"); c->view_brdf = e != 0; return VRHIP_OK; }

int one_upload_mesh_flat(vrhip_ctx* c, const float* bvh, size_t n_bvh_f4, const float* verts,
                           const float* normals, const float* tangents, const float* uvs, size_t n_slots)
{
    if (!c || !bvh || !verts || !normals || !tangents || !uvs) return fail(VRHIP_ERR_INVALID, "null mesh array");
    uint32_t depth = 0, nodes = 0;
    int v = vr::validate_flat(bvh, n_bvh_f4, verts, n_slots, &depth, &nodes);
    if (v != 0) return fail(VRHIP_ERR_BVH, "flattened BVH failed validation (code " + std::to_string(v) + ")");
    if (depth > 62) return fail(VRHIP_ERR_BVH, "BVH deeper than 62 levels");
    vr::DeviceMesh dm;
    std::string why;
    if (!vr::to_device_layout(bvh, n_bvh_f4, (const vr4*)verts, (const vr4*)normals, (const vr4*)tangents,
                              (const vr2*)uvs, dm, why))
        return fail(VRHIP_ERR_BVH, why);
    int rc = set_device(c); if (rc) return rc;
    const size_t nt = dm.tris.size();
    if ((rc = upload(c, c->bvh, dm.nodes.data(), dm.nodes.size() * 16))) return rc;
    if ((rc = upload(c, c->bvh16, dm.nodes16.data(), dm.nodes16.size() * 16))) return rc;
    if ((rc = upload(c, c->verts, dm.tris.data(), nt * sizeof(vr3)))) return rc;
    if ((rc = upload(c, c->tri_e, dm.tri_e.data(), nt * sizeof(vr3)))) return rc;
    if ((rc = upload(c, c->tpath, dm.tpath.data(), dm.tpath.size() * sizeof(unsigned long long)))) return rc;
    if ((rc = upload(c, c->normals, dm.normals.data(), nt * 16))) return rc;
    if ((rc = upload(c, c->tangents, dm.tangents.data(), nt * 16))) return rc;
    if ((rc = upload(c, c->uvs, dm.uvs.data(), nt * 8))) return rc;
    if ((rc = upload(c, c->prim_id, dm.prim_id.data(), dm.prim_id.size() * sizeof(uint32_t)))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    // a host upload keeps no index data: nothing to refit (vrhip_refit_mesh_device)
    dfree(c->slot_vert); dfree(c->node_level); dfree(c->refit_status);
    c->refit_verts = 0;
    c->n_bvh = n_bvh_f4; c->n_slots = n_slots;
    c->bvh_depth = depth; c->bvh_nodes = nodes;
    c->dev_nodes = (uint32_t)(dm.nodes.size() / 4);
    c->dev_tris = (uint32_t)(nt / 3);
    c->mesh = true;
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

// The device builder's entry point (vr_devbvh.hip): the eight arrays of the
// device layout are built from device-resident triangles into fresh buffers and
// swapped into the context only when the build succeeded, so a refused mesh
// leaves the resident one as it was.
namespace {
struct DeviceBuild {
    vr::DevBuildOut o{};
    vr::DevBuildStatus* status = nullptr;
    void* scratch = nullptr;
    ~DeviceBuild()
    {
        dfree(o.bvh); dfree(o.bvh16); dfree(o.verts); dfree(o.tri_e); dfree(o.tpath);
        dfree(o.normals); dfree(o.tangents); dfree(o.uvs); dfree(o.slot_vert); dfree(o.node_level); dfree(o.prim_id); dfree(status);
        if (scratch) (void)hipFree(scratch);
    }
};
} // namespace

int vrhip_upload_mesh_device(vrhip_ctx* c, const float* d_positions, const float* d_normals, const float* d_tangents,
                             const float* d_uvs, uint32_t n_verts, const uint32_t* d_tris, uint32_t n_tris,
                             uint32_t max_leaf_tris)
{
    return vrhip_upload_mesh_device_ex(c, d_positions, d_normals, d_tangents, d_uvs, n_verts, d_tris, n_tris,
                                       max_leaf_tris, VRHIP_DEVBVH_MORTON);
}

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
    vr::DevBuildShape sh = vr::devbvh_shape(n_tris, max_leaf_tris ? max_leaf_tris : 2u);
    if (sah) sh.nodes = sh.n_refs - 1u;           // the worst case: one triangle per leaf
    int rc = set_device(c); if (rc) return rc;
    quiesce(c);
    DeviceBuild b;
    const size_t nv = 3 * (size_t)sh.n_refs;
    HIP_TRY(hipMalloc((void**)&b.o.bvh, 4 * (size_t)sh.nodes * 16));
    HIP_TRY(hipMalloc((void**)&b.o.bvh16, 2 * (size_t)sh.nodes * 16));
    HIP_TRY(hipMalloc((void**)&b.o.verts, nv * sizeof(vr3)));
    HIP_TRY(hipMalloc((void**)&b.o.tri_e, nv * sizeof(vr3)));
    HIP_TRY(hipMalloc((void**)&b.o.tpath, (size_t)sh.n_refs * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc((void**)&b.o.normals, nv * 16));
    HIP_TRY(hipMalloc((void**)&b.o.tangents, nv * 16));
    HIP_TRY(hipMalloc((void**)&b.o.uvs, nv * 8));
    HIP_TRY(hipMalloc((void**)&b.o.slot_vert, nv * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&b.o.node_level, (size_t)sh.nodes * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&b.o.prim_id, (size_t)sh.n_refs * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&b.status, sizeof(vr::DevBuildStatus)));
    HIP_TRY(hipMemsetAsync(b.status, 0, sizeof(vr::DevBuildStatus), c->stream));
    const int e = (sah ? vr::devsah_build : vr::devbvh_build)(d_positions, d_normals, d_tangents, d_uvs, n_verts, d_tris,
                                                              n_tris, max_leaf_tris ? max_leaf_tris : 2u, b.o, b.status,
                                                              &b.scratch, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("device BVH build: ") + hipGetErrorString((hipError_t)e));
    vr::DevBuildStatus st{};
    HIP_TRY(hipMemcpyAsync(&st, b.status, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (st.flags & vr::DEVBVH_BAD_INDEX) return fail(VRHIP_ERR_INVALID, "a triangle index is >= n_verts");
    if (st.flags & vr::DEVBVH_NONFINITE) return fail(VRHIP_ERR_INVALID, "a referenced vertex position is not finite");
    if (st.flags & vr::DEVBVH_BIG_LEAF) return fail(VRHIP_ERR_BVH, "leaf with >= 128 triangles");
    if (st.flags) return fail(VRHIP_ERR_BVH, "device BVH build: internal inconsistency");
    if (sah ? (st.nodes == 0 || st.nodes > sh.nodes || st.leaves != st.nodes + 1u || st.depth == 0 ||
               st.depth > vr::kMaxBuildDepth)
            : (st.depth != sh.depth || st.nodes != sh.nodes || st.leaves != sh.leaves || st.depth > 62))
        return fail(VRHIP_ERR_BVH, "device BVH build: the tree is not the shape its size gives");
    dfree(c->bvh); dfree(c->bvh16); dfree(c->verts); dfree(c->tri_e); dfree(c->tpath);
    dfree(c->normals); dfree(c->tangents); dfree(c->uvs);
    dfree(c->slot_vert); dfree(c->node_level); dfree(c->refit_status); dfree(c->prim_id);
    c->bvh = b.o.bvh; c->bvh16 = b.o.bvh16; c->verts = b.o.verts; c->tri_e = b.o.tri_e; c->tpath = b.o.tpath;
    c->normals = b.o.normals; c->tangents = b.o.tangents; c->uvs = b.o.uvs;
    c->slot_vert = b.o.slot_vert; c->node_level = b.o.node_level; c->refit_status = b.status;
    c->prim_id = b.o.prim_id;
    c->refit_verts = n_verts;
    b.o = vr::DevBuildOut{};
    b.status = nullptr;
    c->n_bvh = 4 * (size_t)st.nodes; c->n_slots = st.slots;
    c->bvh_depth = st.depth; c->bvh_nodes = st.nodes;
    c->dev_nodes = st.nodes;
    c->dev_tris = sh.n_refs;
    c->mesh = true;
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
    if (!c->mesh || c->dev_nodes == 0) return fail(VRHIP_ERR_INVALID, "no mesh loaded");
    if (!c->slot_vert || !c->node_level || !c->refit_status)
        return fail(VRHIP_ERR_INVALID, "the resident mesh was not built on the device (it keeps no index data)");
    if (n_verts != c->refit_verts)
        return fail(VRHIP_ERR_INVALID, "n_verts is " + std::to_string(n_verts) + ", the upload's was " +
                                           std::to_string(c->refit_verts));
    int rc = set_device(c); if (rc) return rc;
    quiesce(c);
    HIP_TRY(hipMemsetAsync(c->refit_status, 0, sizeof(vr::DevBuildStatus), c->stream));
    int e = vr::refit_validate(d_positions, n_verts, c->slot_vert, c->dev_tris, c->refit_status, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("mesh refit: ") + hipGetErrorString((hipError_t)e));
    vr::DevBuildStatus st{};
    HIP_TRY(hipMemcpyAsync(&st, c->refit_status, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (st.flags & vr::DEVBVH_NONFINITE) return fail(VRHIP_ERR_INVALID, "a referenced vertex position is not finite");
    if (st.flags) return fail(VRHIP_ERR_BVH, "mesh refit: internal inconsistency");
    const vr::RefitMesh m{ c->bvh, c->bvh16, c->verts, c->tri_e, c->normals, c->tangents, c->slot_vert, c->node_level,
                           c->dev_tris, c->dev_nodes, c->bvh_depth };
    e = vr::refit_apply(d_positions, d_normals, d_tangents, m, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("mesh refit: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VRHIP_OK;
}

int vrhip_bvh_sah_cost(vrhip_ctx* c, double* cost)
{
    if (!c || !cost) return fail(VRHIP_ERR_INVALID, "null argument");
    if (!c->mesh || c->dev_nodes == 0) return fail(VRHIP_ERR_INVALID, "no mesh loaded");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    const uint32_t nb = vr::refit_cost_blocks(c->dev_nodes);
    double* buf = nullptr;                        // the block partials, then the result
    HIP_TRY(hipMalloc((void**)&buf, ((size_t)nb + 1) * sizeof(double)));
    const int e = vr::refit_sah_cost(c->bvh, c->dev_nodes, buf, buf + nb, c->stream);
    hipError_t he = e ? (hipError_t)e : hipMemcpyAsync(cost, buf + nb, sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    dfree(buf);
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

// Ray queries against the resident mesh (vr_rayquery.hip): the path kernels'
// traversal fed from the caller's ray buffer.  Reads the mesh only; the
// accumulation, the images and the frame counter stay as they are.
static_assert(sizeof(vrhip_ray_hit) == 16 && sizeof(vr::RayHit) == 16, "one 16-B record per ray");
int vrhip_trace_rays(vrhip_ctx* c, const float* d_origins, const float* d_dirs, const float* d_tmax, uint32_t n_rays,
                     uint32_t mode, vrhip_ray_hit* d_hits)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (mode != VRHIP_RAYS_CLOSEST && mode != VRHIP_RAYS_ANY) return fail(VRHIP_ERR_INVALID, "unknown ray query mode");
    if (n_rays > 0 && (!d_origins || !d_dirs || !d_hits)) return fail(VRHIP_ERR_INVALID, "null ray or hit array");
    if (((uintptr_t)d_hits & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_hits is not 16-byte aligned");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_trace_rays");
    if (!c->mesh || c->dev_nodes == 0 || !c->prim_id) return fail(VRHIP_ERR_INVALID, "no mesh loaded");
    if (n_rays == 0) return VRHIP_OK;
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    vr::RenderParams p;
    std::memset(&p, 0, sizeof(p));
    p.bvh = c->bvh; p.bvh16 = c->bvh16; p.tri_e = c->tri_e; p.tpath = c->tpath;
    p.n_nodes = c->dev_nodes; p.n_tris = c->dev_tris;
    p.flags = vr::F_MESH | (c->strict ? (uint32_t)vr::F_STRICT : 0u);
    const vr::RayQuery q{ d_origins, d_dirs, d_tmax, n_rays, mode == VRHIP_RAYS_ANY ? 1u : 0u, c->prim_id,
                          (vr::RayHit*)d_hits };
    // stack entries needed: walk depth + 1 (as build_params, vrhip_render.cpp)
    const int stack = c->bvh_depth <= 15 ? 16 : c->bvh_depth <= 23 ? 24 : c->bvh_depth <= 30 ? 32 : 64;
    const int e = vr::launch_ray_query(p, q, stack, c->cu_count, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("ray query: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
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
    if (!c->mesh || c->dev_nodes == 0) return fail(VRHIP_ERR_INVALID, "no mesh loaded");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    const size_t nv = 3 * (size_t)c->dev_tris;
    std::vector<vr4> dn(4 * (size_t)c->dev_nodes), dnrm(nv), dtan(nv);
    std::vector<vr3> dv(nv);
    std::vector<vr2> duv(nv);
    HIP_TRY(hipMemcpyAsync(dn.data(), c->bvh, dn.size() * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dv.data(), c->verts, nv * sizeof(vr3), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dnrm.data(), c->normals, nv * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dtan.data(), c->tangents, nv * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(duv.data(), c->uvs, nv * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = svc_verify(c)) != VRHIP_OK) return rc;

    vr::FlatMesh flat;
    if (!vr::device_to_flat(dn, dv, dnrm, dtan, duv, flat)) return fail(VRHIP_ERR_BVH, "resident tree is malformed");
    const std::vector<vr4>&ob = flat.bvh, &ov = flat.verts, &on = flat.normals, &ot = flat.tangents;
    const std::vector<vr2>& ou = flat.uvs;
    if (bvh && verts && normals && tangents && uvs) {
        if (*n_bvh_f4 < ob.size() || *n_slots < ov.size()) return fail(VRHIP_ERR_INVALID, "output arrays too small");
        std::memcpy(bvh, ob.data(), ob.size() * 16);
        std::memcpy(verts, ov.data(), ov.size() * 16);
        std::memcpy(normals, on.data(), on.size() * 16);
        std::memcpy(tangents, ot.data(), ot.size() * 16);
        std::memcpy(uvs, ou.data(), ou.size() * 8);
    }
    *n_bvh_f4 = ob.size();
    *n_slots = ov.size();
    return VRHIP_OK;
}

int one_upload_hdr(vrhip_ctx* c, const float* rgba, uint32_t w, uint32_t h)
{
    if (!c || !rgba || w == 0 || h == 0) return fail(VRHIP_ERR_INVALID, "bad hdr arguments");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = upload(c, c->hdr, rgba, (size_t)w * h * 16))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->hdr_w = w; c->hdr_h = h;
    return VRHIP_OK;
}

int one_upload_hdr_half(vrhip_ctx* c, const uint16_t* rgba_half, uint32_t w, uint32_t h)
{
    if (!c || !rgba_half || w == 0 || h == 0) return fail(VRHIP_ERR_INVALID, "bad hdr arguments");
    int rc = set_device(c); if (rc) return rc;
    const size_t n = (size_t)w * h;
    uint16_t* tmp = nullptr;
    HIP_TRY(hipMalloc((void**)&tmp, n * 8));
    quiesce(c);
    dfree(c->hdr);
    if (hipMalloc((void**)&c->hdr, n * 16) != hipSuccess) { dfree(tmp); return fail(VRHIP_ERR_NOMEM, "hdr alloc"); }
    HIP_TRY(hipMemcpyAsync(tmp, rgba_half, n * 8, hipMemcpyHostToDevice, c->stream));
    if (vr::launch_half_to_float(tmp, c->hdr, n, c->stream) != 0) { dfree(tmp); return fail(VRHIP_ERR_HIP, "half convert"); }
    HIP_TRY(hipStreamSynchronize(c->stream));
    dfree(tmp);
    c->hdr_w = w; c->hdr_h = h;
    return VRHIP_OK;
}

int one_upload_texture(vrhip_ctx* c, int type, const float* rgba, uint32_t w, uint32_t h)
{
    if (!c || !rgba || w == 0 || h == 0 || type < 0 || type > 2) return fail(VRHIP_ERR_INVALID, "bad texture arguments");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = upload(c, c->tex[type], rgba, (size_t)w * h * 16))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tex_w[type] = w; c->tex_h[type] = h;
    return VRHIP_OK;
}

int one_upload_brdf(vrhip_ctx* c, const float* table, size_t n_floats)
{
    const size_t n = 90u * 90u * 360u / 2u;    // BRDF_SAMPLING_RES_* (include/vRenderer.h:23-25)
    if (!c || !table || n_floats != 3 * n) return fail(VRHIP_ERR_INVALID, "BRDF table must hold 3*1458000 floats");
    int rc = set_device(c); if (rc) return rc;
    // The device copy is interleaved (entry i's three channels adjacent): one
    // lookup touches one cache line instead of three, 5.8 MB apart.
    std::vector<float> rgb(3 * n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) rgb[3 * i + k] = table[k * n + i];
    if ((rc = upload(c, c->brdf, rgb.data(), 3 * n * sizeof(float)))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VRHIP_OK;
}

int vrhip_load_merl(const char* path, float* table, size_t n_floats)
{
    if (!path || !table || n_floats != vr::kMerlFloats)
        return fail(VRHIP_ERR_INVALID, "BRDF table must hold 3*1458000 floats");
    std::string why;
    if (vr::read_merl(path, table, why) != 0) return fail(VRHIP_ERR_INVALID, why);
    return VRHIP_OK;
}

int vrhip_load_exr(const char* path, uint16_t* rgba_half, size_t n_values, uint32_t* width, uint32_t* height)
{
    if (!path || !width || !height) return fail(VRHIP_ERR_INVALID, "null argument");
    std::vector<uint16_t> px;
    uint32_t w = 0, h = 0;
    std::string why;
    if (vr::read_exr_rgba_half(path, px, w, h, why) != 0) return fail(VRHIP_ERR_INVALID, why);
    *width = w;
    *height = h;
    if (!rgba_half) return VRHIP_OK;                 // size query
    if (n_values < px.size()) return fail(VRHIP_ERR_INVALID, "output too small for 4*w*h half values");
    std::memcpy(rgba_half, px.data(), px.size() * 2);
    return VRHIP_OK;
}

int vrhip_gl_register_image(vrhip_ctx* c, int which, unsigned int gl_texture, unsigned int gl_target)
{
    if (!c || which < 0 || which > 1) return fail(VRHIP_ERR_INVALID, "bad GL registration arguments");
    int rc = set_device(c); if (rc) return rc;
    if (c->gl_res[which]) { HIP_TRY(hipGraphicsUnregisterResource(c->gl_res[which])); c->gl_res[which] = nullptr; }
    const hipError_t e = hipGraphicsGLRegisterImage(&c->gl_res[which], gl_texture, gl_target,
                                                    hipGraphicsRegisterFlagsWriteDiscard);
    if (e != hipSuccess) {
        c->gl_res[which] = nullptr;
        (void)hipGetLastError();        // not sticky: later launches check hipGetLastError
        return fail(VRHIP_ERR_HIP, std::string("hipGraphicsGLRegisterImage: ") + hipGetErrorString(e));
    }
    return VRHIP_OK;
}

int vrhip_gl_present(vrhip_ctx* c)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    int rc = multi_images(c); if (rc) return rc;
    if ((rc = set_device(c)) != VRHIP_OK) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    const void* src[2] = { c->rgba, c->depth };
    for (int i = 0; i < 2; ++i) {
        if (!c->gl_res[i]) continue;
        hipArray_t arr = nullptr;
        HIP_TRY(hipGraphicsMapResources(1, &c->gl_res[i], c->stream));
        hipError_t e = hipGraphicsSubResourceGetMappedArray(&arr, c->gl_res[i], 0, 0);
        if (e == hipSuccess)
            e = hipMemcpy2DToArrayAsync(arr, 0, 0, src[i], (size_t)c->W * 4, (size_t)c->W * 4, c->H,
                                        hipMemcpyDeviceToDevice, c->stream);
        const hipError_t u = hipGraphicsUnmapResources(1, &c->gl_res[i], c->stream);
        if (e != hipSuccess) return fail(VRHIP_ERR_HIP, std::string("GL present: ") + hipGetErrorString(e));
        if (u != hipSuccess) return fail(VRHIP_ERR_HIP, std::string("GL unmap: ") + hipGetErrorString(u));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VRHIP_OK;
}

int vrhip_frame_count(vrhip_ctx* c, uint32_t* frames)
{
    if (!c || !frames) return fail(VRHIP_ERR_INVALID, "null argument");
    *frames = c->frame - 1;
    return VRHIP_OK;
}

static int readback(vrhip_ctx* c, const void* src, void* dst, size_t bytes)
{
    if (!c || !dst) return fail(VRHIP_ERR_INVALID, "null argument");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

int vrhip_read_accum(vrhip_ctx* c, float* out)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (!c->group.empty()) {                          // the accumulation lives on every device: gather it first
        const int rc = multi_gather(c, 1);
        if (rc != VRHIP_OK) return rc;
    }
    return readback(c, c->accum, out, (size_t)c->W * c->H * 16);
}
int vrhip_read_rgba8(vrhip_ctx* c, uint8_t* out)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    const int rc = multi_images(c);
    return rc ? rc : readback(c, c->rgba, out, (size_t)c->W * c->H * 4);
}
int vrhip_read_depth8(vrhip_ctx* c, uint8_t* out)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    const int rc = multi_images(c);
    return rc ? rc : readback(c, c->depth, out, (size_t)c->W * c->H * 4);
}

int vrhip_device_buffers(vrhip_ctx* c, void** accum, void** rgba8, void** depth8)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    const int rc = multi_images(c); if (rc) return rc;       // a group's lead: the whole image first
    if (set_device(c) == VRHIP_OK) (void)svc_close(c);     // the buffers hold every render so far
    // the caller may read them from its own streams: vrhip_sync then waits
    // for the stream's completion (the end of the kernels' write-back)
    c->stream_shared = true;
    if (accum) *accum = c->accum;
    if (rgba8) *rgba8 = c->rgba;
    if (depth8) *depth8 = c->depth;
    return VRHIP_OK;
}

int vrhip_bvh_info(vrhip_ctx* c, uint32_t* depth, uint32_t* n_nodes, uint32_t* n_slots)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (depth) *depth = c->bvh_depth;
    if (n_nodes) *n_nodes = c->bvh_nodes;
    if (n_slots) *n_slots = (uint32_t)c->n_slots;
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
    const bool fill = bvh_out && verts_out && normals_out && tangents_out && uvs_out;
    if (fill) {
        if (*n_bvh_f4 < m.bvh.size() || *n_slots < m.verts.size()) return fail(VRHIP_ERR_INVALID, "output arrays too small");
        std::memcpy(bvh_out, m.bvh.data(), m.bvh.size() * 16);
        std::memcpy(verts_out, m.verts.data(), m.verts.size() * 16);
        std::memcpy(normals_out, m.normals.data(), m.normals.size() * 16);
        std::memcpy(tangents_out, m.tangents.data(), m.tangents.size() * 16);
        std::memcpy(uvs_out, m.uvs.data(), m.uvs.size() * 8);
    }
    *n_bvh_f4 = m.bvh.size();
    *n_slots = m.verts.size();
    return VRHIP_OK;
}

int vrhip_validate_flat(const float* bvh, size_t n_bvh_f4, const float* verts, size_t n_slots,
                        uint32_t* depth, uint32_t* n_nodes)
{
    int v = vr::validate_flat(bvh, n_bvh_f4, verts, n_slots, depth, n_nodes);
    if (v != 0) return fail(VRHIP_ERR_BVH, "validation failed (code " + std::to_string(v) + ")");
    return VRHIP_OK;
}
