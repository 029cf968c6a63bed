// vrhip_scene.cpp -- the context and what it holds besides the mesh
// (vrhip_mesh.cpp): create / destroy, stream, camera and flags, environment /
// texture / BRDF uploads, asset loaders, GL presentation and read-backs
// (include/vrhip.h).
#include <hip/hip_runtime.h>
#include <hip/hip_gl_interop.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "vr_ctx.hpp"
#include "vr_exr.hpp"
#include "vr_merl.hpp"

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
    dfree(c->hdr); dfree(c->tex[0]); dfree(c->tex[1]); dfree(c->tex[2]); dfree(c->brdf);
    for (int i = 0; i < 2; ++i)
        if (c->gl_res[i]) (void)hipGraphicsUnregisterResource(c->gl_res[i]);
    dfree(c->counters); dfree(c->tone_t); dfree(c->dn_planes); dfree(c->dn_frame); dfree(c->atlas_scratch); dfree(c->probe_scratch);
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
    delete c;                                         // the mesh frees its own arrays
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
    dev_ptr<uint16_t> tmp;
    HIP_TRY(dev_alloc(tmp, n * 8));
    quiesce(c);
    dfree(c->hdr);
    if (hipMalloc((void**)&c->hdr, n * 16) != hipSuccess) return fail(VRHIP_ERR_NOMEM, "hdr alloc");
    HIP_TRY(hipMemcpyAsync(tmp.get(), rgba_half, n * 8, hipMemcpyHostToDevice, c->stream));
    if (vr::launch_half_to_float(tmp.get(), c->hdr, n, c->stream) != 0) return fail(VRHIP_ERR_HIP, "half convert");
    HIP_TRY(hipStreamSynchronize(c->stream));
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

std::vector<float> brdf_interleaved(const float* table)
{
    const size_t n = 90u * 90u * 360u / 2u;
    std::vector<float> rgb(3 * n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) rgb[3 * i + k] = table[k * n + i];
    return rgb;
}

int one_upload_brdf(vrhip_ctx* c, const float* table, size_t n_floats)
{
    const size_t n = 90u * 90u * 360u / 2u;    // BRDF_SAMPLING_RES_* (include/vRenderer.h:23-25)
    if (!c || !table || n_floats != 3 * n) return fail(VRHIP_ERR_INVALID, "BRDF table must hold 3*1458000 floats");
    int rc = set_device(c); if (rc) return rc;
    // The device copy is interleaved (entry i's three channels adjacent): one
    // lookup touches one cache line instead of three, 5.8 MB apart.
    const std::vector<float> rgb = brdf_interleaved(table);
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
