// vrhip_multi.cpp -- several GPUs on one image: tile ownership, tile pack and
// unpack, the RCCL gather between ranks (vrhip_comm_*), and the multi-device
// context (vrhip_create_multi) with the public calls that fan out to its members.
#include <cstring>

#include "vr_ctx.hpp"

int vrhip_set_tiling(vrhip_ctx* c, uint32_t rank, uint32_t n_ranks)
{
    if (c && !c->group.empty()) return refuse_multi(c, "vrhip_set_tiling");
    if (!c || n_ranks == 0 || rank >= n_ranks) return fail(VRHIP_ERR_INVALID, "bad tiling");
    // the gather buffers and the RCCL communicator are sized for the
    // communicator's tiling: it cannot change while they exist
    if (c->comm && (rank != c->comm_rank || n_ranks != c->comm_n))
        return fail(VRHIP_ERR_INVALID, "tiling is fixed while a communicator exists (vrhip_comm_destroy first)");
    quiesce(c);
    c->rank = rank; c->nranks = n_ranks;
    return VRHIP_OK;
}

int vrhip_tile_pixels(uint32_t width, uint32_t height, uint32_t rank, uint32_t n_ranks, uint32_t* pix_out,
                      uint32_t* n_pix)
{
    if (!n_pix || n_ranks == 0 || rank >= n_ranks) return fail(VRHIP_ERR_INVALID, "bad tiling arguments");
    const uint32_t tiles_x = width / 16u, n_owned = owned_tiles_of(width, height, rank, n_ranks);
    *n_pix = n_owned * 256u;
    if (pix_out) {
        for (uint32_t j = 0; j < n_owned; ++j) {
            const uint32_t gt = rank + j * n_ranks, ty = tile_row(gt, tiles_x), tx = tile_col(gt, tiles_x, n_ranks);
            for (uint32_t px = 0; px < 256u; ++px)
                pix_out[j * 256u + px] = (ty * 16u + px / 16u) * width + tx * 16u + px % 16u;
        }
    }
    return VRHIP_OK;
}

int vrhip_owned_pixels(vrhip_ctx* c, uint32_t* n_pix)
{
    if (!c || !n_pix) return fail(VRHIP_ERR_INVALID, "null argument");
    *n_pix = owned_tiles_of(c->W, c->H, c->rank, c->nranks) * 256u;
    return VRHIP_OK;
}

static int elem_size(int what) { return what == 1 ? 16 : 4; }
static const void* buf_of(vrhip_ctx* c, int what) { return what == 1 ? (const void*)c->accum : what == 2 ? (const void*)c->depth : (const void*)c->rgba; }

int vrhip_pack_tiles(vrhip_ctx* c, int what, void* dst)
{
    if (!c || !dst || what < 0 || what > 2) return fail(VRHIP_ERR_INVALID, "bad pack arguments");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    int e = vr::launch_pack_tiles(buf_of(c, what), dst, (uint32_t)elem_size(what), c->W, c->W / 16u,
                                  owned_tiles_of(c->W, c->H, c->rank, c->nranks), c->rank, c->nranks, 0, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, "pack launch failed");
    return VRHIP_OK;
}

int vrhip_unpack_tiles(vrhip_ctx* c, int what, const void* src, uint32_t n_ranks, size_t stride_bytes)
{
    if (!c || !src || what < 0 || what > 2 || n_ranks == 0) return fail(VRHIP_ERR_INVALID, "bad unpack arguments");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    if (stride_bytes) {                   // one launch for every rank's buffer
        const int e = vr::launch_unpack_ranks(src, const_cast<void*>(buf_of(c, what)), (uint32_t)elem_size(what), c->W,
                                              c->W / 16u, (c->W / 16u) * (c->H / 16u), 0u, n_ranks, stride_bytes,
                                              c->stream);
        if (e) return fail(VRHIP_ERR_HIP, "unpack launch failed");
        return VRHIP_OK;
    }
    const char* s = (const char*)src;      // tightly packed: buffers of different lengths, one launch each
    for (uint32_t r = 0; r < n_ranks; ++r) {
        const uint32_t n_owned = owned_tiles_of(c->W, c->H, r, n_ranks);
        int e = vr::launch_pack_tiles(s, const_cast<void*>(buf_of(c, what)), (uint32_t)elem_size(what), c->W,
                                      c->W / 16u, n_owned, r, n_ranks, 1, c->stream);
        if (e) return fail(VRHIP_ERR_HIP, "unpack launch failed");
        s += (size_t)n_owned * 256u * elem_size(what);
    }
    return VRHIP_OK;
}

// ---- multi-GPU tile gather over RCCL ------------------------
static int nccl_fail(ncclResult_t r, const char* what)
{
    return fail(VRHIP_ERR_COMM, std::string(what) + ": " + ncclGetErrorString(r));
}

static uint32_t max_owned_pixels(uint32_t W, uint32_t H, uint32_t n_ranks)
{
    return owned_tiles_of(W, H, 0, n_ranks) * 256u;       // rank 0 owns the most tiles
}

int vrhip_comm_unique_id(uint8_t id[VRHIP_COMM_ID_BYTES])
{
    if (!id) return fail(VRHIP_ERR_INVALID, "id is NULL");
    static_assert(VRHIP_COMM_ID_BYTES == sizeof(ncclUniqueId), "ncclUniqueId size");
    ncclUniqueId u;
    const ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) return nccl_fail(r, "ncclGetUniqueId");
    std::memcpy(id, &u, sizeof(u));
    return VRHIP_OK;
}

int vrhip_comm_init(vrhip_ctx* c, uint32_t rank, uint32_t n_ranks, const uint8_t id[VRHIP_COMM_ID_BYTES])
{
    if (c && !c->group.empty()) return refuse_multi(c, "vrhip_comm_init");
    if (!c || !id || n_ranks == 0 || rank >= n_ranks) return fail(VRHIP_ERR_INVALID, "bad communicator arguments");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    if (c->comm) { (void)ncclCommDestroy(c->comm); c->comm = nullptr; }
    dfree(c->comm_send); dfree(c->comm_recv);
    if ((rc = vrhip_set_tiling(c, rank, n_ranks)) != VRHIP_OK) return rc;
    c->comm_rank = rank; c->comm_n = n_ranks;
    c->comm_slot = (size_t)max_owned_pixels(c->W, c->H, n_ranks) * 16u;
    const size_t slot = c->comm_slot ? c->comm_slot : 16u;
    if (hipMalloc((void**)&c->comm_send, slot) != hipSuccess ||
        (rank == 0 && hipMalloc((void**)&c->comm_recv, slot * n_ranks) != hipSuccess))
        return fail(VRHIP_ERR_NOMEM, "gather buffers");
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    const ncclResult_t r = ncclCommInitRank(&c->comm, (int)n_ranks, u, (int)rank);   // blocks until every rank joins
    if (r != ncclSuccess) { c->comm = nullptr; return nccl_fail(r, "ncclCommInitRank"); }
    return VRHIP_OK;
}

int vrhip_comm_gather(vrhip_ctx* c, int what)
{
    if (c && !c->group.empty()) {                     // the group's own communicators
        if (what < 0 || what > 2) return fail(VRHIP_ERR_INVALID, "bad gather arguments");
        return multi_gather(c, what);
    }
    if (!c || what < 0 || what > 2) return fail(VRHIP_ERR_INVALID, "bad gather arguments");
    if (!c->comm) return fail(VRHIP_ERR_INVALID, "vrhip_comm_init has not been called");
    int rc = set_device(c); if (rc) return rc;
    if (c->service > 0 && c->svc.open && c->svc.posted > 0 && c->svc.fin.staging) {
        // explicit service mode only: inside a session the image after its
        // last launch is staged by the session's finish pass and gathered
        // when the session closes (the caller syncs before any host-side
        // wait on the other ranks, include/vrhip.h).  In automatic mode the
        // gather closes the session and is enqueued now (below, through
        // vrhip_pack_tiles), so no rank's collective waits on a host call
        c->svc.fin.gather[c->svc.posted - 1u] |= 1u << what;
        c->svc.gathers.emplace_back(c->svc.posted - 1u, what);
        ++c->svc_deferred;
        return VRHIP_OK;
    }
    // pack -> gather -> (rank 0) unpack, all on the context stream, behind the
    // finish passes that wrote the images
    if (c->rank != c->comm_rank || c->nranks != c->comm_n)
        return fail(VRHIP_ERR_INVALID, "tiling differs from the communicator's");
    const size_t bytes = (size_t)max_owned_pixels(c->W, c->H, c->nranks) * (size_t)elem_size(what);
    if (bytes > c->comm_slot) return fail(VRHIP_ERR_INVALID, "gather payload exceeds the communicator's buffers");
    if ((rc = vrhip_pack_tiles(c, what, c->comm_send)) != VRHIP_OK) return rc;
    const ncclResult_t r = ncclGather(c->comm_send, c->comm_recv, bytes, ncclUint8, 0, c->comm, c->stream);
    if (r != ncclSuccess) return nccl_fail(r, "ncclGather");
    if (c->rank == 0) return vrhip_unpack_tiles(c, what, c->comm_recv, c->nranks, bytes);
    return VRHIP_OK;
}

int vrhip_comm_destroy(vrhip_ctx* c)
{
    if (c && !c->group.empty()) return refuse_multi(c, "vrhip_comm_destroy");
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->comm) {
        const ncclResult_t r = ncclCommDestroy(c->comm);
        c->comm = nullptr;
        if (r != ncclSuccess) return nccl_fail(r, "ncclCommDestroy");
    }
    dfree(c->comm_send); dfree(c->comm_recv);
    return VRHIP_OK;
}

// ---- multi-device renderer (SURVEY 8b create_multi) -------------------------
// One vrhip_ctx over several GPUs of this process: a member context per
// device, each owning the 16x16 tiles i, i + n, ... of the image; the RCCL
// communicators made in one call (ncclCommInitAll); every setting and upload
// fanned out; vrhip_render renders every device's tiles and gathers the RGBA8
// and depth tiles to the lead device (one grouped ncclGather each), whose
// images are then the whole frame (read-back, GL presentation).  The
// reference's single caller creates one renderer (src/NGLScene.cpp:82-89):
// through this context it drives all the devices named in VRHIP_DEVICES
// (integration/vRendererHIP.cpp).

template <typename F>
static int fanout(vrhip_ctx* c, F&& f)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (c->group.empty()) return f(c);
    for (vrhip_ctx* m : c->group) {
        const int rc = f(m);
        if (rc != VRHIP_OK) return rc;
    }
    return VRHIP_OK;
}

int refuse_multi(vrhip_ctx*, const char* what)
{
    return fail(VRHIP_ERR_INVALID, std::string(what) + " is not available on a multi-device context (vrhip_create_multi)");
}

// every member's `what` tiles to the lead: pack on each member's stream, one
// grouped ncclGather (one thread drives all ranks), unpack on the lead
int multi_gather(vrhip_ctx* c, int what)
{
    const size_t esz = what == 1 ? 16u : 4u;
    const size_t bytes = (size_t)max_owned_pixels(c->W, c->H, (uint32_t)c->group.size()) * esz;
    int rc;
    for (vrhip_ctx* m : c->group) {
        if ((rc = set_device(m)) != VRHIP_OK) return rc;
        if ((rc = svc_close(m)) != VRHIP_OK) return rc;
        if ((rc = vr::launch_pack_tiles(buf_of(m, what), m->comm_send, (uint32_t)esz, m->W, m->W / 16u,
                                        owned_tiles_of(m->W, m->H, m->rank, m->nranks), m->rank, m->nranks, 0,
                                        m->stream)) != 0)
            return fail(VRHIP_ERR_HIP, "pack launch failed");
    }
    ncclResult_t r = ncclGroupStart();
    if (r != ncclSuccess) return nccl_fail(r, "ncclGroupStart");
    for (vrhip_ctx* m : c->group) {
        r = ncclGather(m->comm_send, m->comm_recv, bytes, ncclUint8, 0, m->comm, m->stream);
        if (r != ncclSuccess) { (void)ncclGroupEnd(); return nccl_fail(r, "ncclGather"); }
    }
    r = ncclGroupEnd();
    if (r != ncclSuccess) return nccl_fail(r, "ncclGroupEnd");
    if ((rc = set_device(c)) != VRHIP_OK) return rc;
    const uint32_t n = (uint32_t)c->group.size();
    if (n > 1 && vr::launch_unpack_ranks(c->comm_recv + bytes, const_cast<void*>(buf_of(c, what)), (uint32_t)esz,
                                         c->W, c->W / 16u, (c->W / 16u) * (c->H / 16u), 1u, n, bytes, c->stream) != 0)
        return fail(VRHIP_ERR_HIP, "unpack launch failed");       // (the lead's own tiles are in place)
    return VRHIP_OK;
}

// The lead's colour and depth images after the last render: the members'
// render-service sessions close and their RGBA8 and depth tiles are gathered
// (two grouped ncclGathers), once per run of render calls -- so back-to-back
// renders with no read in between keep their sessions open across calls.
int multi_images(vrhip_ctx* c)
{
    if (!c || c->group.empty() || !c->group_stale) return VRHIP_OK;
    int rc = multi_gather(c, 0);
    if (rc == VRHIP_OK) rc = multi_gather(c, 2);
    if (rc == VRHIP_OK) c->group_stale = false;
    return rc;
}

int vrhip_create_multi(const int* devices, uint32_t n_devices, uint32_t width, uint32_t height, vrhip_ctx** out)
{
    if (!out || !devices || n_devices == 0 || n_devices > 64)
        return fail(VRHIP_ERR_INVALID, "bad multi-device arguments (1..64 devices)");
    *out = nullptr;
    for (uint32_t i = 0; i < n_devices; ++i)
        for (uint32_t j = 0; j < i; ++j)
            if (devices[i] == devices[j]) return fail(VRHIP_ERR_INVALID, "a device appears twice");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(VRHIP_ERR_NO_DEVICE, "no HIP device");
    for (uint32_t i = 0; i < n_devices; ++i)
        if (devices[i] < 0 || devices[i] >= n) return fail(VRHIP_ERR_INVALID, "device index out of range");
    std::vector<vrhip_ctx*> ms(n_devices, nullptr);
    auto undo = [&](int code) {
        for (vrhip_ctx* m : ms)
            if (m) { m->group.clear(); vrhip_destroy(m); }
        return code;
    };
    int rc;
    for (uint32_t i = 0; i < n_devices; ++i) {
        if ((rc = vrhip_create(devices[i], width, height, &ms[i])) != VRHIP_OK) return undo(rc);
        ms[i]->rank = i; ms[i]->nranks = n_devices;
    }
    std::vector<ncclComm_t> comms(n_devices, nullptr);
    const ncclResult_t r = ncclCommInitAll(comms.data(), (int)n_devices, devices);
    if (r != ncclSuccess) return undo(nccl_fail(r, "ncclCommInitAll"));
    const size_t slot = (size_t)max_owned_pixels(width, height, n_devices) * 16u;
    for (uint32_t i = 0; i < n_devices; ++i) {
        vrhip_ctx* m = ms[i];
        m->comm = comms[i];
        m->comm_rank = i; m->comm_n = n_devices; m->comm_slot = slot;
        if ((rc = set_device(m)) != VRHIP_OK) return undo(rc);
        if (hipMalloc((void**)&m->comm_send, slot ? slot : 16u) != hipSuccess ||
            (i == 0 && hipMalloc((void**)&m->comm_recv, (slot ? slot : 16u) * n_devices) != hipSuccess))
            return undo(fail(VRHIP_ERR_NOMEM, "gather buffers"));
    }
    ms[0]->group = ms;
    (void)set_device(ms[0]);
    *out = ms[0];
    return VRHIP_OK;
}

int vrhip_device_group(vrhip_ctx* c, uint32_t* n_devices, int* devices)
{
    if (!c || !n_devices) return fail(VRHIP_ERR_INVALID, "null argument");
    const uint32_t n = c->group.empty() ? 1u : (uint32_t)c->group.size();
    if (devices)
        for (uint32_t i = 0; i < n; ++i) devices[i] = c->group.empty() ? c->device : c->group[i]->device;
    *n_devices = n;
    return VRHIP_OK;
}

int vrhip_set_camera(vrhip_ctx* c, const float origin[3], const float dir[3], const float up[3], const float right[3],
                     float fov_scale)
{ return fanout(c, [&](vrhip_ctx* m) { return one_set_camera(m, origin, dir, up, right, fov_scale); }); }
int vrhip_clear(vrhip_ctx* c) { return fanout(c, [&](vrhip_ctx* m) { return one_clear(m); }); }
int vrhip_set_fresnel(vrhip_ctx* c, float coef, float power)
{ return fanout(c, [&](vrhip_ctx* m) { return one_set_fresnel(m, coef, power); }); }
int vrhip_use_cornell_box(vrhip_ctx* c, int e) { return fanout(c, [&](vrhip_ctx* m) { return one_use_cornell_box(m, e); }); }
int vrhip_use_example_sphere(vrhip_ctx* c, int e) { return fanout(c, [&](vrhip_ctx* m) { return one_use_example_sphere(m, e); }); }
int vrhip_set_strict_traversal(vrhip_ctx* c, int e) { return fanout(c, [&](vrhip_ctx* m) { return one_set_strict_traversal(m, e); }); }
int vrhip_use_brdf(vrhip_ctx* c, int e) { return fanout(c, [&](vrhip_ctx* m) { return one_use_brdf(m, e); }); }
// (vrhip_upload_mesh_flat prepares the arrays once, then fans out itself: vrhip_mesh.cpp)
int vrhip_upload_hdr(vrhip_ctx* c, const float* rgba, uint32_t w, uint32_t h)
{ return fanout(c, [&](vrhip_ctx* m) { return one_upload_hdr(m, rgba, w, h); }); }
int vrhip_upload_hdr_half(vrhip_ctx* c, const uint16_t* rgba_half, uint32_t w, uint32_t h)
{ return fanout(c, [&](vrhip_ctx* m) { return one_upload_hdr_half(m, rgba_half, w, h); }); }
int vrhip_upload_texture(vrhip_ctx* c, int type, const float* rgba, uint32_t w, uint32_t h)
{ return fanout(c, [&](vrhip_ctx* m) { return one_upload_texture(m, type, rgba, w, h); }); }
int vrhip_upload_brdf(vrhip_ctx* c, const float* table, size_t n_floats)
{ return fanout(c, [&](vrhip_ctx* m) { return one_upload_brdf(m, table, n_floats); }); }
int vrhip_set_overlap(vrhip_ctx* c, int mode) { return fanout(c, [&](vrhip_ctx* m) { return one_set_overlap(m, mode); }); }
int vrhip_set_path_split(vrhip_ctx* c, uint32_t groups) { return fanout(c, [&](vrhip_ctx* m) { return one_set_path_split(m, groups); }); }
int vrhip_set_service(vrhip_ctx* c, int mode) { return fanout(c, [&](vrhip_ctx* m) { return one_set_service(m, mode); }); }
int vrhip_set_kernel_timing(vrhip_ctx* c, int on) { return fanout(c, [&](vrhip_ctx* m) { return one_set_kernel_timing(m, on); }); }
int vrhip_set_sync_flag(vrhip_ctx* c, int on) { return fanout(c, [&](vrhip_ctx* m) { return one_set_sync_flag(m, on); }); }
int vrhip_sync(vrhip_ctx* c)
{
    const int rc = multi_images(c);                  // a group: the lead's images are complete after a sync
    return rc ? rc : fanout(c, [&](vrhip_ctx* m) { return one_sync(m); });
}

int vrhip_render(vrhip_ctx* c, uint32_t n_frames, const uint32_t* times, uint32_t time_seed)
{
    if (!c || c->group.empty()) return one_render(c, n_frames, times, time_seed);
    // every device renders its tiles (asynchronously, on its own render
    // service when calls come back to back); the colour and depth tiles go to
    // the lead when its images are next needed (multi_images: read-back, GL
    // present, device buffers, sync)
    for (vrhip_ctx* m : c->group) {
        const int rc = one_render(m, n_frames, times, time_seed);
        if (rc != VRHIP_OK) return rc;
    }
    c->group_stale = true;
    return VRHIP_OK;
}
