// vrhip_service.cpp -- render service sessions (vrhip_set_service).
//
// Back-to-back render calls on mesh scenes (vrhip_set_service: automatically
// behind a launch still in flight for the launches that overlap on the path
// streams -- shards and small frames -- or always) post their launches to
// ONE persistent kernel (vr_kernel.hpp service_body) through a descriptor
// ring in host-pinned memory, so a launch's drain overlaps the next launch's
// paths.  Each launch writes its paths' results to its own scratch slot; when
// the session closes -- at the next call that is not a render (sync, read-back,
// upload, any setting or buffer access: svc_close), when its slots are full,
// or when a launch does not fit the session -- one finish pass sums every
// pixel's paths launch by launch in path order, stages the images of
// launches whose gather was deferred (vrhip_comm_gather inside a session),
// and the gathers run.  Results are bit-identical to launch-by-launch
// rendering; only their time of arrival changes.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "vr_ctx.hpp"

#ifndef VR_SVC_IDLE_MS
#define VR_SVC_IDLE_MS 20            // the kernel retires after this long without a new launch
#endif
#ifndef VR_SVC_POST_MS
#define VR_SVC_POST_MS 5             // the host posts to a session only within this of its last post
#endif

void svc_free(vrhip_ctx* c)
{
    auto& S = c->svc;
    if (S.s) (void)hipStreamSynchronize(S.s);
    for (int i = 0; i < 2; ++i) {
        if (S.rings[i]) (void)hipHostFree(S.rings[i]);
        if (S.ring_done[i]) (void)hipEventDestroy(S.ring_done[i]);
        S.rings[i] = S.rings_dev[i] = nullptr;
        S.ring_done[i] = nullptr;
        S.ring_used[i] = false;
    }
    S.host = nullptr;
    dfree(S.dev); dfree(S.qctl); dfree(S.scratch); dfree(S.prim); dfree(S.staging); dfree(S.subs);
    S.qctl_slots = S.scratch_cap = S.prim_cap = S.staging_cap = S.subs_cap = 0;
    if (S.k0) (void)hipEventDestroy(S.k0);
    if (S.k1) (void)hipEventDestroy(S.k1);
    if (S.finished) (void)hipEventDestroy(S.finished);
    if (S.summed) (void)hipEventDestroy(S.summed);
    if (S.s) (void)hipStreamDestroy(S.s);
    S.k0 = S.k1 = S.finished = S.summed = nullptr;
    S.summed_valid = false;
    S.s = nullptr;
    S.open = false;
}

// The launch parameters that must stay fixed within a session (scene,
// camera, flags, tiling, frame buffers): per-launch fields cleared.
static vr::RenderParams svc_key(const vr::RenderParams& p)
{
    vr::RenderParams k = p;
    k.first_frame = k.n_frames = 0;
    std::memset(k.times, 0, sizeof(k.times));
    k.split = k.use_scratch = k.small_blocks = k.inline_prim = 0;
    k.paths = nullptr; k.path_w = nullptr; k.prim = nullptr; k.chunk_ctr = nullptr;
    k.path_cost = nullptr; k.sub_cost = nullptr; k.sub_order = nullptr; k.order_cap = 0;
    k.counters = nullptr; k.n_queues = 0;
    return k;
}

// Launch slots a session of launches of up to kmax frames gets (0 or 1:
// the service cannot take such launches; they take the launch path).  The
// scratch budget (VRHIP_SERVICE_BYTES, default 24 GiB of the 288 GiB HBM)
// holds every slot's path results: 24 B per pixel and frame.
uint32_t svc_slots(const vrhip_ctx* c, uint32_t path_stride, uint32_t kmax, size_t* slot_bytes_out)
{
    const size_t stride = path_stride;
    const size_t slot_bytes = ((12u * 2u * (size_t)kmax * stride + 4u * stride) + 255u) & ~(size_t)255u;
    static const size_t env_budget = [] {
        const char* e = std::getenv("VRHIP_SERVICE_BYTES");
        return e ? (size_t)std::atoll(e) : ((size_t)24 << 30);
    }();
    const size_t budget = c->svc_budget ? c->svc_budget : env_budget;
    if (slot_bytes_out) *slot_bytes_out = slot_bytes;
    return (uint32_t)std::min<size_t>(vr::kSvcMaxLaunches, budget / slot_bytes);
}

// The kernel of ring ri's last session has finished: it must have consumed
// every launch the session's finish pass summed (svc_post's hand-shake makes
// that so; this check makes any breach loud instead of a silently wrong image).
static int svc_check_ring(vrhip_ctx* c, uint32_t ri)
{
    auto& S = c->svc;
    if (!S.ring_used[ri] || S.ring_checked[ri] || (S.open && S.cur_ring == ri)) return VRHIP_OK;
    HIP_TRY(hipEventSynchronize(S.ring_done[ri]));
    S.ring_checked[ri] = true;
    const uint32_t r = __atomic_load_n(&S.rings[ri]->retired, __ATOMIC_ACQUIRE);
    if ((r & vr::kSvcClosed) == 0u || (r & ~vr::kSvcClosed) < S.ring_posted[ri])
        return fail(VRHIP_ERR_HIP, "render service: the kernel consumed " + std::to_string(r & ~vr::kSvcClosed) +
                                       " of " + std::to_string(S.ring_posted[ri]) + " launches");
    return VRHIP_OK;
}
// after a host synchronisation: both rings' finished sessions
int svc_verify(vrhip_ctx* c)
{
    int rc;
    for (uint32_t ri = 0; ri < 2; ++ri)
        if ((rc = svc_check_ring(c, ri)) != VRHIP_OK) return rc;
    return VRHIP_OK;
}

// Closes the open session: the kernel retires once the ring is drained, then
// the finish pass and the deferred gathers run on `stream`.  Asynchronous.
int svc_close(vrhip_ctx* c)
{
    auto& S = c->svc;
    c->flag_armed = 0;                  // every call that queues work closes the session first
    if (!S.open) return VRHIP_OK;
    S.open = false;
    __atomic_store_n(&S.host->closed, 1u, __ATOMIC_RELEASE);
    S.ring_posted[S.cur_ring] = S.posted;
    S.ring_checked[S.cur_ring] = false;
    HIP_TRY(hipStreamWaitEvent(c->stream, S.k1, 0));
    // the launches the host posted and the kernel took (svc_post): a launch
    // that met a retiring kernel was not counted and went the launch path.
    // A session that took none has nothing to sum: no finish pass (on a fresh
    // accumulation it would tonemap with a frame count of 0) and no gathers
    // (a gather is deferred only behind a launch the session took)
    S.fin.n = S.posted;
    if (S.posted > 0) {
        const int e = vr::launch_service_finish(S.p, S.fin, S.n_tiles, c->stream);
        if (e != 0) return fail(VRHIP_ERR_HIP, std::string("service finish launch: ") + hipGetErrorString((hipError_t)e));
    }
    if (!S.gathers.empty()) {
        HIP_TRY(hipEventRecord(S.summed, c->stream));
        S.summed_epoch = c->stream_epoch;
        S.summed_valid = true;
    }
    // deferred gathers, in call order; rank 0 keeps its own tiles from the
    // finish pass (the final state) and unpacks the other ranks' of every gather
    for (const auto& g : S.gathers) {
        const int what = g.second;
        const size_t esz = what == 1 ? 16u : 4u;
        const size_t off = what == 0 ? 0u : what == 2 ? 4u * (size_t)S.fin.stage_pixels : 8u * (size_t)S.fin.stage_pixels;
        const uint8_t* send = S.staging + (size_t)g.first * S.fin.stage_bytes + off;
        const size_t bytes = (size_t)S.fin.stage_pixels * esz;
        const ncclResult_t r = ncclGather(send, c->comm_recv, bytes, ncclUint8, 0, c->comm, c->stream);
        if (r != ncclSuccess) return fail(VRHIP_ERR_COMM, std::string("ncclGather: ") + ncclGetErrorString(r));
        if (c->rank == 0 && c->nranks > 1) {
            void* dst = what == 1 ? (void*)c->accum : what == 2 ? (void*)c->depth : (void*)c->rgba;
            const int ee = vr::launch_unpack_ranks(c->comm_recv + bytes, dst, (uint32_t)esz, c->W, c->W / 16u,
                                                   (c->W / 16u) * (c->H / 16u), 1u, c->nranks, bytes, c->stream);
            if (ee) return fail(VRHIP_ERR_HIP, "unpack launch failed");
        }
    }
    S.gathers.clear();
    HIP_TRY(hipEventRecord(S.finished, c->stream));
    S.finished_used = true;
    // vrhip_last_kernel_ms after a session: its span, kernel start to finish pass
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    c->timed = true;
    c->flag_synced = false;
    // the session's kernel span: one span covering all its launches
    hipEvent_t a = nullptr, b = nullptr;
    if ((a = S.k0) && (b = S.k1)) {
        S.k0 = S.k1 = nullptr;
        c->kev_pending.push_back({ a, b, S.posted });
    }
    return VRHIP_OK;
}

// Opens a session for launches of up to kmax frames with parameters p.
int svc_open(vrhip_ctx* c, const vr::RenderParams& p, int stack, uint32_t n_tiles, uint32_t kmax)
{
    auto& S = c->svc;
    if (!S.s) {
        HIP_TRY(hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&S.finished, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&S.summed, hipEventDisableTiming));
        for (int i = 0; i < 2; ++i) {
            HIP_TRY(hipHostMalloc((void**)&S.rings[i], sizeof(vr::SvcHostCtl), hipHostMallocCoherent | hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer((void**)&S.rings_dev[i], S.rings[i], 0));
            HIP_TRY(hipEventCreateWithFlags(&S.ring_done[i], hipEventDisableTiming));
        }
        HIP_TRY(hipMalloc((void**)&S.dev, sizeof(vr::SvcDevCtl)));
    }
    // this session's ring: the other one's kernel may still run; this one's
    // kernel (two sessions back) must have retired before the host rewrites it
    const uint32_t ri = S.ring_i;
    S.ring_i ^= 1u;
    int rc;
    if (S.ring_used[ri]) {
        HIP_TRY(hipEventSynchronize(S.ring_done[ri]));
        if ((rc = svc_check_ring(c, ri)) != VRHIP_OK) return rc;
    }
    const size_t stride = p.path_stride;
    size_t slot_bytes = 0;
    uint32_t slots = svc_slots(c, p.path_stride, kmax, &slot_bytes);
    const uint32_t stage_px = owned_tiles_of(c->W, c->H, 0, c->nranks) * 256u;   // rank 0 owns the most tiles
    // staged images serve deferred gathers only, which need a communicator
    // (vrhip_comm_init closes any open session, so none appears mid-session)
    const size_t stage_bytes = c->comm ? (24u * (size_t)stage_px + 255u) & ~(size_t)255u : 0u;
    // the slots' scratch grows into at most half of the device memory free
    // now (plus what the session already holds): several contexts or ranks
    // on one GPU share it, and the launch path needs its own scratch
    if (slots >= 2 && (size_t)slots * slot_bytes > S.scratch_cap) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const size_t avail = (free_b + S.scratch_cap + S.staging_cap) / 2u;
            slots = (uint32_t)std::min<size_t>(slots, avail / (slot_bytes + stage_bytes));
        }
        (void)hipGetLastError();
    }
    if (slots < 2) return fail(VRHIP_ERR_NOMEM, "render service: device memory holds fewer than 2 launch slots");
    auto grow = [&](auto*& ptr, size_t& cap, size_t need) -> int {
        if (need <= cap) return VRHIP_OK;
        // the previous session's kernel and finish pass may still use the old buffer
        if (S.s) HIP_TRY(hipStreamSynchronize(S.s));
        if (S.finished_used) HIP_TRY(hipEventSynchronize(S.finished));
        dfree(ptr);
        cap = 0;
        const hipError_t e = hipMalloc((void**)&ptr, need);
        if (e != hipSuccess) {
            ptr = nullptr;
            (void)hipGetLastError();
            return fail(VRHIP_ERR_NOMEM, std::string("render service scratch: ") + hipGetErrorString(e));
        }
        cap = need;
        return VRHIP_OK;
    };
    if ((rc = grow(S.scratch, S.scratch_cap, (size_t)slots * slot_bytes)) != VRHIP_OK) return rc;
    if ((rc = grow(S.prim, S.prim_cap, 32u * stride)) != VRHIP_OK) return rc;
    if (stage_bytes && (rc = grow(S.staging, S.staging_cap, (size_t)slots * stage_bytes)) != VRHIP_OK) return rc;
    if ((rc = grow(S.qctl, S.qctl_slots, (size_t)slots * vr::kSvcQctlWords * 4u)) != VRHIP_OK) return rc;
    // HDRI scenes: escaped camera rays' pixels leave the session's paths (F_SPARSE)
    const bool sparse = !c->cornell && (p.flags & vr::F_STRICT) == 0u;
    if (sparse && (rc = grow(S.subs, S.subs_cap, 4u * stride)) != VRHIP_OK) return rc;
    if (!S.k0 && (rc = take_event(c, &S.k0)) != VRHIP_OK) return rc;
    if (!S.k1 && (rc = take_event(c, &S.k1)) != VRHIP_OK) return rc;
    S.slot_bytes = slot_bytes; S.slots = slots; S.kmax = kmax; S.posted = 0;
    S.stack = stack; S.n_tiles = n_tiles;
    S.p = p;
    S.p.paths = reinterpret_cast<vr3*>(S.scratch);
    S.p.prim = S.prim;
    S.p.sparse_px = sparse ? S.subs : nullptr;
    S.host = S.rings[ri];
    S.cur_ring = ri;
    S.p.svc_host = S.rings_dev[ri]; S.p.svc_dev = S.dev; S.p.svc_qctl = S.qctl;
    S.p.svc_slot_bytes = slot_bytes; S.p.svc_kmax = kmax;
    S.p.svc_idle_ticks = (c->svc_idle_us ? c->svc_idle_us : (uint32_t)VR_SVC_IDLE_MS * 1000u) * 100u;   // 100 MHz
    S.key = svc_key(p);
    std::memset(&S.fin, 0, sizeof(S.fin));
    S.fin.first_frame = c->frame;
    S.fin.staging = stage_bytes ? S.staging : nullptr; S.fin.stage_bytes = stage_bytes; S.fin.stage_pixels = stage_px;
    S.gathers.clear();
    // the ring: nothing posted, open, the kernel serving (the kernel launch
    // below orders these host stores before the kernel's first read)
    S.host->posted = 0; S.host->closed = 0; S.host->retired = 0;
    // everything queued on `stream` first (uploads, clears, earlier finish
    // passes) -- or, when the last thing queued there that this session's
    // kernels depend on is the previous session's finish pass (its scratch,
    // primary records and pixel list are reused here), only that: its
    // deferred gathers then run beside this session (Session::summed)
    if (S.summed_valid && S.summed_epoch == c->stream_epoch) {
        HIP_TRY(hipStreamWaitEvent(S.s, S.summed, 0));
    } else {
        HIP_TRY(hipEventRecord(c->ev_join, c->stream));
        HIP_TRY(hipStreamWaitEvent(S.s, c->ev_join, 0));
    }
    S.summed_valid = false;
    HIP_TRY(hipMemsetAsync(S.dev, 0, sizeof(vr::SvcDevCtl), S.s));
    HIP_TRY(hipMemsetAsync(S.qctl, 0, (size_t)slots * vr::kSvcQctlWords * 4u, S.s));
    HIP_TRY(hipEventRecord(S.k0, S.s));
    HIP_TRY(hipEventRecord(c->ev0, S.s));
    c->ev0_valid = true;
    const int e = vr::launch_service(S.p, n_tiles, stack, S.s);
    if (e != 0) return fail(VRHIP_ERR_HIP, std::string("service launch: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipEventRecord(S.k1, S.s));
    HIP_TRY(hipEventRecord(S.ring_done[ri], S.s));
    S.ring_used[ri] = true;
    S.ring_checked[ri] = false;
    S.ring_posted[ri] = 0;
    S.open = true;
    ++c->svc_sessions;
    S.last_post = std::chrono::steady_clock::now();
    return VRHIP_OK;
}

// Posts one launch of k frames (first frame c->frame) to the open session.
// false: the session's kernel was retiring (idle) and did not take it -- the
// caller closes the session without it and renders it another way.  The
// hand-shake with svc_ring_wave: the host stores `posted`, fences, reads
// `retired`; the kernel stores `retired`, fences, reads `posted`.  Whichever
// store is first, the other side's load sees it, so the launch is taken by
// the kernel (it saw `posted`) or by the caller (it saw `retired`) -- never
// by neither.
bool svc_post(vrhip_ctx* c, uint32_t k, const uint32_t* times, uint32_t time_seed)
{
    auto& S = c->svc;
    vr::SvcLaunch& d = S.host->desc[S.posted];
    d.first_frame = c->frame;
    d.n_frames = k;
    for (uint32_t i = 0; i < k; ++i) d.times[i] = times ? times[i] : time_seed;
    __atomic_store_n(&S.host->posted, S.posted + 1u, __ATOMIC_SEQ_CST);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    if (__atomic_load_n(&S.host->retired, __ATOMIC_SEQ_CST) != 0u) return false;
    S.fin.n_frames[S.posted] = k;
    ++S.posted;
    ++c->svc_served;
    S.last_post = std::chrono::steady_clock::now();
    return true;
}

// Whether the open session can take a launch of k frames with parameters p.
bool svc_fits(const vrhip_ctx* c, const vr::RenderParams& p, uint32_t k)
{
    const auto& S = c->svc;
    if (!S.open || S.posted >= S.slots || k > S.kmax) return false;
    const auto idle = std::chrono::steady_clock::now() - S.last_post;
    const uint32_t window_us = c->svc_window_us ? c->svc_window_us : (uint32_t)VR_SVC_POST_MS * 1000u;
    if (idle > std::chrono::microseconds(window_us)) return false;
    const vr::RenderParams key = svc_key(p);
    return std::memcmp(&key, &S.key, sizeof(key)) == 0;
}

int one_set_service(vrhip_ctx* c, int mode)
{
    if (!c || mode < -1 || mode > 1) return fail(VRHIP_ERR_INVALID, "bad service mode");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    c->service = mode;
    return VRHIP_OK;
}

int vrhip_set_service_timing(vrhip_ctx* c, uint32_t idle_us, uint32_t post_window_us, uint32_t post_delay_us)
{
    if (c && !c->group.empty()) return refuse_multi(c, "vrhip_set_service_timing");
    if (!c || idle_us > 10000000u || post_window_us > 10000000u || post_delay_us > 10000000u)
        return fail(VRHIP_ERR_INVALID, "bad service timing (each at most 10 s)");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    c->svc_idle_us = idle_us; c->svc_window_us = post_window_us; c->svc_post_delay_us = post_delay_us;
    return VRHIP_OK;
}

int vrhip_set_service_budget(vrhip_ctx* c, size_t bytes)
{
    if (c && !c->group.empty()) return refuse_multi(c, "vrhip_set_service_budget");
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    c->svc_budget = bytes;
    return VRHIP_OK;
}

int vrhip_service_stats(vrhip_ctx* c, uint64_t* refused_launches)
{
    if (!c || !refused_launches) return fail(VRHIP_ERR_INVALID, "null argument");
    *refused_launches = c->svc_refused;
    return VRHIP_OK;
}

int vrhip_service_info(vrhip_ctx* c, uint64_t out[VRHIP_SERVICE_INFO])
{
    if (!c || !out) return fail(VRHIP_ERR_INVALID, "null argument");
    out[0] = c->svc_refused;
    out[1] = c->svc_sessions;
    out[2] = c->svc_served;
    out[3] = c->svc_deferred;
    out[4] = c->svc_alloc_fallbacks;
    return VRHIP_OK;
}
