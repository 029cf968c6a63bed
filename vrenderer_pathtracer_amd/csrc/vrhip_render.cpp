// vrhip_render.cpp -- vrhip_render and what a render call needs: the launch
// decisions and launches (render_impl), the path streams' scratch, the
// one-frame graph, kernel-time accounting, vrhip_sync and its completion flag.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "vr_ctx.hpp"

// Launches of at most this many paths per pixel trace the camera ray in the
// path kernel instead of a separate primary pass (RenderParams::inline_prim).
#ifndef VR_INLINE_PRIM_PATHS
#define VR_INLINE_PRIM_PATHS 2
#endif

// the finish pass's arrival counters: vr::kSyncGroups group words 256 B apart, then the top word
constexpr size_t kSyncCtrBytes = (64u * vr::kSyncGroups + 64u) * sizeof(uint32_t);
// Largest finish pass that carries the completion flag (tiles of 16x16):
// counting a 3840x2160 pass's 32,400 block arrivals cost more than the flag
// saves (C5 one frame per call +0.6 %, r06zt)
#ifndef VR_SYNC_FLAG_MAX_TILES
#define VR_SYNC_FLAG_MAX_TILES 8192
#endif

constexpr int kDebugSlots = vr::kExecCounterBase + vr::kExecCounters;

static int ensure_counters(vrhip_ctx* c)
{
    if (!c->counters) {
        HIP_TRY(hipMalloc((void**)&c->counters, sizeof(unsigned long long) * kDebugSlots));
        HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(unsigned long long) * kDebugSlots, c->stream));
    }
    return VRHIP_OK;
}

// Adds the render-kernel times of completed launches to the totals; with
// `wait`, waits for all of them.  Never blocks otherwise, so a render call
// does not wait for the previous one (launches pipeline, see render_impl).
// Launches on the path streams can overlap and need not start in queue
// order: every span is placed on one time line (ms after kev_origin) and
// the total is the length of the union of the spans, so it never exceeds the
// wall time they cover and is never less than the longest span.
static int account_pending(vrhip_ctx* c, bool wait)
{
    while (!c->kev_pending.empty()) {
        auto pr = c->kev_pending.front();
        if (wait) {
            HIP_TRY(hipEventSynchronize(pr.second));
        } else {
            const hipError_t q = hipEventQuery(pr.second);
            if (q == hipErrorNotReady) break;
            if (q != hipSuccess) return fail(VRHIP_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
        }
        bool keep_start = false;
        if (!c->kev_origin) { c->kev_origin = pr.first; keep_start = true; }
        float t0 = 0.f, t1 = 0.f;
        HIP_TRY(hipEventElapsedTime(&t0, c->kev_origin, pr.first));
        HIP_TRY(hipEventElapsedTime(&t1, c->kev_origin, pr.second));
        if (t1 > t0) {
            // insert [t0, t1) and merge the intervals it touches
            auto& u = c->kev_union;
            double lo = t0, hi = t1;
            std::vector<std::pair<double, double>> out;
            out.reserve(u.size() + 1);
            for (const auto& iv : u) {
                if (iv.second < lo || iv.first > hi) out.push_back(iv);
                else { lo = std::min(lo, iv.first); hi = std::max(hi, iv.second); }
            }
            out.emplace_back(lo, hi);
            std::sort(out.begin(), out.end());
            u.swap(out);
        }
        c->launches_total += pr.launches;
        c->kev_pending.pop_front();
        if (!keep_start) c->kev_free.push_back(pr.first);
        c->kev_free.push_back(pr.second);
    }
    double tot = 0.0;
    for (const auto& iv : c->kev_union) tot += iv.second - iv.first;
    c->kernel_ms_total = tot;
    return VRHIP_OK;
}

int take_event(vrhip_ctx* c, hipEvent_t* e)
{
    if (!c->kev_free.empty()) { *e = c->kev_free.back(); c->kev_free.pop_back(); return VRHIP_OK; }
    HIP_TRY(hipEventCreate(e));
    return VRHIP_OK;
}

// Path groups per pixel for a sphere-only launch of n_tiles tiles x k frames
// (mesh scenes use the path-pool kernel: no groups).  A thread runs its
// pixel's paths back to back; with one group it accumulates them in registers
// (no result scratch, no finish pass), so one group is the choice whenever
// the launch has blocks enough to fill the GPU, and for one-frame launches
// (2 paths per thread: little imbalance to hide).  Otherwise the paths are
// split into the smallest power of two of groups that gives 16 blocks per CU
// (four resident blocks per CU, four rounds).  Measured (1xMI355X, 16-frame
// steps, scripts/split_sweep.py): C4 (8,040 tiles) split 1 0.634 ms, 2 0.638,
// 4 0.639, 8 0.678; one frame per call 0.089 ms against 0.105-0.145; C1
// (1,024 tiles) split 1 0.434, 2 0.319, 4 0.296, 8 0.299, 16 0.310; one frame
// per call 0.062 (split 1) against 0.068.
// Sphere-only HDRI scenes (C4): path groups per pixel at least this many.
// Their pixels split into camera-ray escapes -- one result for all paths,
// stored once (kSharedMissW) -- and the few on the example sphere, whose 2K
// paths (BRDF lookups, HDRI fetches: dependent gathers) one thread would run
// back to back, the launch's critical path.  C4 at 16 frames per launch
// (r04, scripts/c4_probe.py): 1 group 0.470 ms, 2 0.323, 4 0.246, 8 0.253,
// 16 0.362 (every group recomputes the camera ray and sphere tests).
#ifndef VR_SPHERE_SPLIT
#define VR_SPHERE_SPLIT 4
#endif
static uint32_t choose_split(const vrhip_ctx* c, uint32_t n_tiles, uint32_t k, bool shared_escape)
{
    uint32_t t = c->path_split;
    if (t == 0) {
        const uint32_t target = c->cu_count * 16u;
        t = 1;
        if (k > 1)
            while (n_tiles * t < target && t < 2u * k) t *= 2;
        // (launches of 4 frames or more: one frame per call keeps its 2 paths
        // in one thread -- direct accumulation, no finish pass: C4 0.084 ms
        // per frame against 0.093 with 2 groups)
        if (shared_escape && k >= 4) t = std::max<uint32_t>(t, VR_SPHERE_SPLIT);
    }
    return std::max<uint32_t>(1u, std::min<uint32_t>(t, 2u * k));
}

// Entries per XCD in a longest-first order list: the most sub-tiles one XCD's
// bands (vr::kXcdBands sub-tiles each, dealt round-robin to 8 XCDs) can hold.
static size_t order_cap(size_t n_sub) { return (n_sub / (8u * vr::kXcdBands) + 1u) * vr::kXcdBands; }

// Scratch of one path stream, allocated when the stream is first used and
// grown when a launch needs more (growing waits for every reader first).
static int ensure_lane(vrhip_ctx* c, vrhip_ctx::Lane& l, size_t need, uint32_t path_stride)
{
    const size_t prim_need = 2 * (size_t)path_stride;
    if ((l.paths && need > l.paths_cap) || (l.prim && prim_need > l.prim_cap)) {
        quiesce(c);                                       // the finish passes read the scratch too
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (need > l.paths_cap) {
        dfree(l.paths);
        l.paths_cap = 0;
        HIP_TRY(hipMalloc((void**)&l.paths, need * sizeof(vr4)));
        l.paths_cap = need;
    }
    if (prim_need > l.prim_cap) {
        dfree(l.prim);
        l.prim_cap = 0;
        HIP_TRY(hipMalloc((void**)&l.prim, prim_need * sizeof(vr4)));
        l.prim_cap = prim_need;
    }
    const size_t n_sub = path_stride / 64u;
    if (path_stride > l.px_cap) {                         // the F_SPARSE pixel list: one word per owned pixel
        dfree(l.px_list);
        l.px_cap = 0;
        HIP_TRY(hipMalloc((void**)&l.px_list, (size_t)path_stride * sizeof(uint32_t)));
        l.px_cap = path_stride;
    }
    if (n_sub > l.sub_cap) {                              // the order buffers hold 8 XCD lists of order_cap(n_sub)
        l.sub_cap = 0;
        for (int i = 0; i < 2; ++i) {
            dfree(l.sub_cost[i]); dfree(l.sub_order[i]);
            l.order_nsub[i] = 0;
            HIP_TRY(hipMalloc((void**)&l.sub_cost[i], n_sub * sizeof(uint32_t)));
            HIP_TRY(hipMalloc((void**)&l.sub_order[i], 8u * order_cap(n_sub) * sizeof(uint32_t)));
        }
        l.sub_cap = n_sub;
    }
    if (!l.chunk_ctr) {
        const size_t bytes = sizeof(uint32_t) * vr::kQueueStride * (VR_MAX_QUEUES + 1);   // heads + drained-queue mask
        HIP_TRY(hipMalloc((void**)&l.chunk_ctr, bytes));
        HIP_TRY(hipMemsetAsync(l.chunk_ctr, 0, bytes, c->stream));

        HIP_TRY(hipEventRecord(c->ev_join, c->stream));
        HIP_TRY(hipStreamWaitEvent(l.s, c->ev_join, 0));
    }
    return VRHIP_OK;
}

// One-frame launches as a HIP graph (VRHIP_GRAPH=1, experiment): the path
// kernel and the finish pass of a synchronous one-frame call, captured from
// the context stream once per longest-first order slot (the slots' order and
// cost buffers differ), re-captured when any launch parameter but the
// frame's number and seed changes, and launched with those two kernel nodes'
// arguments updated -- one graph launch instead of two kernel launches
// between the host's wake-up and the next frame's path kernel.
static int one_frame_graph(vrhip_ctx* c, const vr::RenderParams& p, uint32_t n_tiles, int stack, uint32_t gi)
{
    auto& G = c->fgraph[gi];
    vr::RenderParams key = p;
    key.first_frame = 0;
    std::memset(key.times, 0, sizeof(key.times));
    if (!G.valid || std::memcmp(&key, &G.key, sizeof(key)) != 0) {
        if (G.x) { (void)hipGraphExecDestroy(G.x); G.x = nullptr; }
        if (G.g) { (void)hipGraphDestroy(G.g); G.g = nullptr; }
        G.valid = false;
        HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        const int e1 = vr::launch_render(p, n_tiles, stack, 0, c->stream);
        const int e2 = vr::launch_finish(p, n_tiles, c->stream);
        const hipError_t ec = hipStreamEndCapture(c->stream, &G.g);
        if (e1 || e2 || ec != hipSuccess)
            return fail(VRHIP_ERR_HIP, std::string("one-frame graph capture: ") +
                                           hipGetErrorString(ec != hipSuccess ? ec : (hipError_t)(e1 ? e1 : e2)));
        size_t n = 0;
        HIP_TRY(hipGraphGetNodes(G.g, nullptr, &n));
        std::vector<hipGraphNode_t> nodes(n);
        HIP_TRY(hipGraphGetNodes(G.g, nodes.data(), &n));
        int k = 0;
        for (size_t i = 0; i < n; ++i) {
            hipGraphNodeType t;
            HIP_TRY(hipGraphNodeGetType(nodes[i], &t));
            if (t != hipGraphNodeTypeKernel) continue;
            if (k == 2) return fail(VRHIP_ERR_HIP, "one-frame graph: more than two kernel nodes");
            G.kn[k] = nodes[i];
            HIP_TRY(hipGraphKernelNodeGetParams(nodes[i], &G.kp[k]));
            ++k;
        }
        if (k != 2) return fail(VRHIP_ERR_HIP, "one-frame graph: expected the path kernel and the finish pass");
        HIP_TRY(hipGraphInstantiate(&G.x, G.g, nullptr, nullptr, 0));
        G.key = key;
        G.valid = true;
        ++c->graph_captures;
    }
    G.arg = p;
    void* args[1] = { &G.arg };
    for (int k = 0; k < 2; ++k) {
        hipKernelNodeParams kp = G.kp[k];
        kp.kernelParams = args;
        kp.extra = nullptr;
        HIP_TRY(hipGraphExecKernelNodeSetParams(G.x, G.kn[k], &kp));
    }
    HIP_TRY(hipGraphLaunch(G.x, c->stream));
    ++c->graph_launches;
    return VRHIP_OK;
}

// VRHIP_QUEUES: work-queue heads for experiments (a power of two, 8..VR_MAX_QUEUES; 0: not set)
static uint32_t env_queues()
{
    static const uint32_t env_q = [] {
        const char* e = std::getenv("VRHIP_QUEUES");
        const uint32_t q = e ? (uint32_t)std::atoi(e) : 0u;
        return (q >= 8 && q <= (uint32_t)VR_MAX_QUEUES && (q & (q - 1)) == 0) ? q : 0u;
    }();
    return env_q;
}

// What the launches of one render call share.
struct RenderCall {
    vr::RenderParams p;          // the launch parameters (build_params; per-launch fields set launch by launch)
    uint32_t n_frames;
    const uint32_t* times;
    uint32_t time_seed;
    int count;                   // 0 production, 1 reference-algorithm counting variant, 2 instrumented production kernels
    uint32_t n_tiles;            // 16x16 tiles this rank owns
    int stack;                   // traversal stack entries
    uint32_t k_max;              // frames of the call's largest launch
    uint32_t split_max;
    size_t need;                 // scratch float4s of the largest launch
    bool wave_kernel;            // mesh scenes: the path-pool kernel (scratch + finish pass)
};

// The launch parameters that come from the context: camera, scene
// (scene_params), frame buffers, tiling, and the traversal stack depth.
static void build_params(const vrhip_ctx* c, RenderCall& q)
{
    vr::RenderParams& p = q.p;
    std::memset(&p, 0, sizeof(p));
    camera_params(c, p);
    p.tone_t = c->tone_t;
    p.wr = (c->W / 16u) * 16u; p.hr = rendered_rows(c);
    scene_params(c, p);
    p.tiles_x = p.wr / 16u;
    p.rank = c->rank; p.nranks = c->nranks;
    p.accum = c->accum; p.rgba = c->rgba; p.depth = c->depth;
    q.n_tiles = owned_tiles_of(c->W, c->H, c->rank, c->nranks);
    q.stack = mesh_stack_entries(c->mesh.a.depth);
    q.wave_kernel = (p.flags & vr::F_MESH) != 0u;
}

// The service attempt: whether this call's launches go to the render service
// (vrhip_service.cpp), and if so the posting of them.  *done: the frames the
// service took; the launch path takes the rest.  Counting launches and
// anything else than a production mesh launch end a session first.
static int serve(vrhip_ctx* c, RenderCall& q, uint32_t* done)
{
    vr::RenderParams& p = q.p;
    int rc;
    // the call's largest launch, against the mesh limits of the launch loop's
    // overlap (launch_decisions: no sphere-scene term here, the service takes mesh launches only)
    const size_t paths_kmax = (size_t)p.path_stride * 2u * q.k_max;
    const bool ovl_size_mesh = paths_kmax < ((size_t)1 << 24) || (c->nranks > 1 && paths_kmax < ((size_t)1 << 25));
    const bool in_flight = c->svc.open || (c->timed && !c->flag_synced && hipEventQuery(c->ev1) == hipErrorNotReady);
    // whole frames take the service too: back-to-back launches then
    // overlap each other's drain and share one primary pass (r04 A/B,
    // 16-frame steps, bit-identical: C3 16,505 -> 18,948, C5 21,630 ->
    // 22,171 Mpaths/s; r05, the 7-wave Cornell service kernel: C2 4,185
    // -> 4,313 at 16 frames per step; on the 6-wave kernel of round 4 they
    // lost, 4,111 -> 4,021)
    // (Cornell-box scenes with material features run a feature-class
    // service kernel at 6 waves: C2D's whole frames 3,710 -> 3,687 on it,
    // so they keep the launch path)
    const bool c2_exact = p.flags == (vr::F_CORNELL | vr::F_MESH);
    const bool svc_size = ovl_size_mesh || !c->cornell || c2_exact;
    // a session's images arrive with the finish pass its CLOSE enqueues, at a
    // later library call: a caller that holds the stream or the buffers
    // (stream_shared) queues its own reads right behind vrhip_render and must
    // find the results there, so its context joins a session only when it
    // asked for one (mode 1) -- the rule the completion flag follows
    // (launch_decisions)
    const bool svc_auto = c->service < 0 && !c->stream_shared && svc_size && in_flight && c->overlap != 0;
    // launches whose slots the scratch budget cannot hold twice take the
    // launch path in every mode (4K frames of many frames per launch)
    const bool svc = q.count == 0 && q.wave_kernel && q.stack <= 32 && q.n_tiles > 0 &&
                     (c->service > 0 || svc_auto) &&
                     svc_slots(c, p.path_stride, q.k_max, nullptr) >= 2u;
    if (!svc) return svc_close(c);
    p.n_queues = c->cornell ? VR_QUEUES : VR_QUEUES_HDRI;
    if (env_queues()) p.n_queues = env_queues();
    while (*done < q.n_frames) {
        const uint32_t k = std::min<uint32_t>(q.n_frames - *done, (uint32_t)vr::kMaxFramesPerLaunch);
        if (c->svc.open && !svc_fits(c, p, k) && (rc = svc_close(c)) != VRHIP_OK) return rc;
        if (!c->svc.open && (rc = svc_open(c, p, q.stack, q.n_tiles, q.k_max)) != VRHIP_OK) {
            // no scratch for the session's slots (memory shared with
            // other contexts or ranks): this call's remaining frames
            // take the launch path, which needs one launch's scratch
            if (rc != VRHIP_ERR_NOMEM) return rc;
            ++c->svc_alloc_fallbacks;
            return VRHIP_OK;
        }
        // (the test hook's delay: only before posts after a session's
        // first -- the first post meets a kernel that just started)
        if (c->svc_post_delay_us && c->svc.posted > 0)
            std::this_thread::sleep_for(std::chrono::microseconds(c->svc_post_delay_us));
        if (!svc_post(c, k, q.times ? q.times + *done : nullptr, q.time_seed)) {
            // the session's kernel retired as this launch was posted:
            // close the session without it; this call's remaining
            // frames take the launch path
            if ((rc = svc_close(c)) != VRHIP_OK) return rc;
            ++c->svc_refused;
            return VRHIP_OK;
        }
        c->frame += k;
        *done += k;
    }
    c->last_split = 1; c->last_use_scratch = 1; c->last_kind = 2;
    return VRHIP_OK;
}

// What one launch of the launch path decides before it queues anything (its split, scratch use, block
// size, camera-ray mode and queue heads go straight into the launch parameters).
// small: under 2^24 paths (one frame per call, shards): 256-thread blocks.
// in_flight: a launch is still running (this call's previous one, or the last call's).  Automatic overlap
//   only behind one: a launch submitted to an idle device (one frame per synchronous call) runs its render
//   and finish kernels on `stream` with no cross-stream waits.
// ovl_size: small enough for automatic overlap: under 2^24 paths, and under 2^25 for a rank's shard (C5's
//   8-way shards of 33 M paths: 8-rank projection 0.757 -> 0.78 of linear); whole 720p frames of 29.5 M
//   paths lose with it (C2 -1.7 %, C3 -6 %: two persistent launches contend), as do C5's 66 M-path 4-way
//   shards (-17 %); sphere scenes (render_kernel, no path pool) overlap up to 2^27 paths: C4's 66 M-path
//   launches 299 -> 481 G paths/s (r04; C3 -6 %, C5 -14 % forced, so meshes keep the limit) -- one launch's
//   tail and finish pass run under the next.
// ovl: the launch takes the next of the VR_PATH_STREAMS path streams: launch i's render kernels wait only
//   for the finish pass of launch i - 3 (the last reader of the same scratch), so they start while launch
//   i-1 drains its longest paths -- and are not held up by launch i-1's finish pass, which itself waits for
//   CUs until that drain.  The finish passes run in order on `stream`.  Without overlap every launch uses
//   the same path stream, so it waits for the previous one (and its finish pass) like a single stream.
//   Counting launches never overlap: their counters are zeroed on `stream`, which a path stream would not
//   wait for, and they accumulate in place.
// sparse: HDRI mesh launches with a primary pass skip the pixels whose camera ray escapes: one shared
//   result each, the path kernel over the pixels whose camera ray hits (F_SPARSE, vr_kernel.hpp primary_kernel).
// on_lane: overlapped launches run on the lane's path stream, the others on `stream` (in order behind
//   everything queued there).
// order: longest-first: launches whose drain is a large share of them (one frame per call) measure per
//   sub-tile costs and take their sub-tiles in the order the previous launch on this scratch measured.
// graph: a synchronous one-frame call's path kernel + finish pass as one graph launch (VRHIP_GRAPH).
// arm: a call of one launch on `stream` on a context whose stream nobody else uses: its finish pass is the
//   last work on `stream`, so it can carry the completion flag a following vrhip_sync polls.
struct LaunchPlan {
    uint32_t k;                  // frames
    bool small, in_flight, ovl_size, ovl, sparse, on_lane, order, timed, graph, arm;
};

static LaunchPlan launch_decisions(const vrhip_ctx* c, const RenderCall& q, vr::RenderParams& p, uint32_t done)
{
    LaunchPlan d{};
    const uint32_t k = d.k = std::min<uint32_t>(q.n_frames - done, (uint32_t)vr::kMaxFramesPerLaunch);
    const int count = q.count;
    p.first_frame = c->frame;
    p.n_frames = k;
    p.split = std::min<uint32_t>(q.split_max, 2u * k);
    // the reference counting variant, and sphere-only launches whose
    // pixels run all their paths in one thread (split 1), accumulate in
    // registers in path order (render_kernel's direct mode): no scratch
    // round trip, no finish pass
    p.use_scratch = (count == 1 || (!q.wave_kernel && p.split == 1u)) ? 0u : 1u;
    for (uint32_t i = 0; i < k; ++i) p.times[i] = q.times ? q.times[done + i] : q.time_seed;
    const size_t paths_k = (size_t)p.path_stride * 2u * k;
    d.small = paths_k < ((size_t)1 << 24);
    d.in_flight = done > 0 || (c->timed && !c->flag_synced && hipEventQuery(c->ev1) == hipErrorNotReady);
    d.ovl_size = paths_k < ((size_t)1 << 24) || (c->nranks > 1 && paths_k < ((size_t)1 << 25)) ||
                 (!q.wave_kernel && paths_k < ((size_t)1 << 27));
    d.ovl = count == 0 && (c->overlap > 0 || (c->overlap < 0 && d.ovl_size && d.in_flight));
    p.small_blocks = d.small ? 1u : 0u;
    // (owned pixels < 2^31: the textured one-frame kernels pack the path
    // index into the pixel slot, vr_kernel.hpp wave_body)
    p.inline_prim = (2u * k <= (uint32_t)VR_INLINE_PRIM_PATHS && count != 1 && p.path_stride < (1u << 31)) ? 1u : 0u;
    d.sparse = q.wave_kernel && !c->cornell && count != 1 && (p.flags & vr::F_STRICT) == 0u && !p.inline_prim;
    // (launches over the listed pixels of HDRI scenes -- a fifth of the
    // paths, all of them mesh paths -- take VR_QUEUES like the Cornell
    // box: C3 16 / 32 / 64 heads 16,630 / 16,408 / 16,172 Mpaths/s, r04)
    p.n_queues = paths_k < ((size_t)1 << 25) ? ((c->cornell || d.sparse) ? VR_QUEUES : VR_QUEUES_HDRI) : VR_QUEUES_LARGE;
    if (env_queues()) p.n_queues = env_queues();
    d.on_lane = p.use_scratch && d.ovl;
    d.order = q.wave_kernel && d.small && count == 0 && c->cost_order && p.inline_prim;
    // per-launch span events (vrhip_kernel_stats) only with kernel timing
    // on (vrhip_set_kernel_timing): recorded on the stream around the
    // render kernels they cost ≈ 8 µs per synchronous one-frame call
    d.timed = q.n_tiles && c->kernel_timing;
    // (a rank without a tile launches nothing: there is no kernel node to capture)
    d.graph = c->use_graph && count == 0 && q.wave_kernel && k == 1u && !d.on_lane && !d.timed && p.inline_prim &&
              p.use_scratch && q.n_tiles > 0;
    d.arm = c->sync_flag_mode && count == 0 && k == q.n_frames && done == 0 && !d.on_lane && p.use_scratch &&
            q.n_tiles > 0 && q.n_tiles <= VR_SYNC_FLAG_MAX_TILES && !c->comm && c->group.empty() && !c->stream_shared;
    return d;
}

// The lane's scratch, order slots and the waits of a launch that uses scratch
// (on render stream rs) for everything that last read or wrote them.
static int prepare_lane(vrhip_ctx* c, const RenderCall& q, const LaunchPlan& d, vr::RenderParams& p,
                        vrhip_ctx::Lane& l, hipStream_t rs)
{
    int rc;
    // launches that overlap: every path stream's
    // scratch at once -- a lane first used behind a launch in flight
    // would otherwise allocate there (hipMalloc waits for the device)
    // and serialise the overlapped launches; whole frames run on lane 0
    // (only where overlap can happen: never with vrhip_set_overlap(0))
    const bool all_lanes = d.ovl_size && c->overlap != 0 && q.count == 0;
    for (auto& ln : c->lane)
        if ((all_lanes || &ln == &l) && (rc = ensure_lane(c, ln, q.need, p.path_stride)) != VRHIP_OK) return rc;
    if (d.ovl) c->parity = (c->parity + 1u) % VR_PATH_STREAMS;
    p.paths = reinterpret_cast<vr::vr3*>(l.paths); p.path_w = reinterpret_cast<float*>(p.paths + q.need);
    p.prim = l.prim; p.chunk_ctr = l.chunk_ctr;
    p.sparse_px = d.sparse ? l.px_list : nullptr;
    const uint32_t n_sub = p.path_stride / 64u;
    // per-path costs after the radiances and depth terms in the scratch
    // (need x 16 B holds need x 12 + path_stride x 4 + need x 1)
    p.path_cost = d.order ? reinterpret_cast<uint8_t*>(p.path_w + p.path_stride) : nullptr;
    // VRHIP_ORDER_SLOTS=1 (measurement): one slot, the previous launch's order
    static const uint32_t order_slots = [] {
        const char* e = std::getenv("VRHIP_ORDER_SLOTS");
        return (e && std::atoi(e) == 1) ? 1u : 2u;
    }();
    const uint32_t w = order_slots == 2u ? l.oi : 0u;
    p.sub_cost = d.order ? l.sub_cost[w] : nullptr;
    p.sub_order = (d.order && l.order_nsub[w] == n_sub) ? l.sub_order[w] : nullptr;
    p.order_cap = (uint32_t)order_cap(n_sub);
    if (d.on_lane && l.used) HIP_TRY(hipStreamWaitEvent(rs, l.finished, 0));
    // the order pass of this slot (it read the slot's costs, which this
    // launch's finish pass rewrites, and wrote the order this launch
    // reads); a launch that does not order waits for both slots
    for (uint32_t i = 0; i < 2u; ++i) {
        if ((i == w || !d.order) && l.order_pending[i]) {
            HIP_TRY(hipStreamWaitEvent(rs, l.ordered[i], 0));
            l.order_pending[i] = false;
        }
    }
    return VRHIP_OK;
}

// The launch's kernels and events: the render kernels on rs between the span
// events, the finish pass on `stream` (or both as the one-frame graph), and
// the order pass behind it on the lane's stream.
static int issue_launch(vrhip_ctx* c, const RenderCall& q, const LaunchPlan& d, vr::RenderParams& p,
                        vrhip_ctx::Lane& l, hipStream_t rs)
{
    int rc;
    hipEvent_t k0 = nullptr, k1 = nullptr;
    if (d.timed) {
        if ((rc = take_event(c, &k0)) != VRHIP_OK || (rc = take_event(c, &k1)) != VRHIP_OK) return rc;
        c->kev_pending.push_back({ k0, k1, 1u });
        HIP_TRY(hipEventRecord(k0, rs));
    }
    if (q.count != 1) {               // production and its instrumented copy (same shape)
        c->last_split = p.split; c->last_use_scratch = p.use_scratch;
        c->last_kind = q.wave_kernel ? 1u : 0u;
    }
    if (d.graph) {
        const uint32_t gi = (p.sub_cost && p.sub_cost == l.sub_cost[1]) ? 1u : 0u;
        if ((rc = one_frame_graph(c, p, q.n_tiles, q.stack, gi)) != VRHIP_OK) return rc;
        c->last_kind = 3u;
    } else {
        int e = vr::launch_render(p, q.n_tiles, q.stack, q.count, rs);
        if (e != 0) return fail(VRHIP_ERR_HIP, std::string("render launch: ") + hipGetErrorString((hipError_t)e));
        if (k1) HIP_TRY(hipEventRecord(k1, rs));
        if (d.on_lane) {
            HIP_TRY(hipEventRecord(l.done, rs));
            HIP_TRY(hipStreamWaitEvent(c->stream, l.done, 0));
        }
        if (d.arm) {
            if (!c->sync_flag) {
                HIP_TRY(hipHostMalloc((void**)&c->sync_flag, 64, hipHostMallocCoherent | hipHostMallocMapped));
                *c->sync_flag = 0u;
            }
            if (!c->sync_ctr) {
                HIP_TRY(hipMalloc((void**)&c->sync_ctr, kSyncCtrBytes));
                HIP_TRY(hipMemsetAsync(c->sync_ctr, 0, kSyncCtrBytes, c->stream));
            }
            if (++c->sync_seq == 0u) c->sync_seq = 1u;
            p.sync_flag = c->sync_flag; p.sync_ctr = c->sync_ctr; p.sync_seq = c->sync_seq;
        }
        e = vr::launch_finish(p, q.n_tiles, c->stream);
        if (e != 0) return fail(VRHIP_ERR_HIP, std::string("finish launch: ") + hipGetErrorString((hipError_t)e));
        if (d.arm) c->flag_armed = p.sync_seq;
        p.sync_flag = nullptr; p.sync_ctr = nullptr;
    }
    if (p.use_scratch) {
        HIP_TRY(hipEventRecord(l.finished, c->stream));
        l.used = true;
    }
    if (p.path_cost) {
        // the next launch but one on this scratch takes this launch's
        // order (the slots alternate): sorted on the path stream behind
        // this finish pass, off the context stream, so a synchronous
        // caller waits for it neither here nor at its next launch
        const uint32_t w = p.sub_cost == l.sub_cost[0] ? 0u : 1u;
        HIP_TRY(hipStreamWaitEvent(l.s, l.finished, 0));
        const int e = vr::launch_order(p.sub_cost, l.sub_order[w], p.path_stride / 64u, p.order_cap, l.s);
        if (e != 0) return fail(VRHIP_ERR_HIP, std::string("order launch: ") + hipGetErrorString((hipError_t)e));
        HIP_TRY(hipEventRecord(l.ordered[w], l.s));
        l.order_pending[w] = true;
        l.order_nsub[w] = p.path_stride / 64u;
        l.oi = w ^ 1u;
    }
    return VRHIP_OK;
}

// count: 0 production, 1 reference-algorithm counting variant (in place, no
// scratch), 2 instrumented production kernels (same launch shape as 0)
static int render_impl(vrhip_ctx* c, uint32_t n_frames, const uint32_t* times, uint32_t time_seed, int count)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (n_frames == 0) return VRHIP_OK;
    if (!c->cornell && !c->hdr)
        return fail(VRHIP_ERR_NO_ENV, "HDRI mode needs an environment map (vrhip_upload_hdr)");
    int rc = set_device(c); if (rc) return rc;
    c->flag_armed = 0;
    RenderCall q;
    q.n_frames = n_frames; q.times = times; q.time_seed = time_seed; q.count = count;
    build_params(c, q);
    vr::RenderParams& p = q.p;
    if (count) {
        if ((rc = ensure_counters(c)) != VRHIP_OK) return rc;
        HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(unsigned long long) * kDebugSlots, c->stream));
        p.counters = c->counters;
    }
    q.k_max = std::min<uint32_t>(n_frames, (uint32_t)vr::kMaxFramesPerLaunch);
    // sphere-only HDRI scenes: camera-ray escapes share one result (render_kernel)
    const bool shared_escape = (p.flags & (vr::F_MESH | vr::F_CORNELL)) == 0u;
    q.split_max = count == 1 ? 1u : choose_split(c, q.n_tiles, q.k_max, shared_escape);
    p.path_stride = q.n_tiles * (uint32_t)vr::kBlockThreads;
    q.need = (size_t)2 * q.k_max * p.path_stride;
    // the path-pool kernel is persistent: one resident set of blocks per CU
    // (the launcher sizes it from the kernel's occupancy) draining the work queues
    p.wave_blocks = c->cu_count;
    // VRHIP_WAVES_PER_SIMD: cap the path kernel's resident waves (experiments)
    static const uint32_t env_waves = [] {
        const char* e = std::getenv("VRHIP_WAVES_PER_SIMD");
        return e ? (uint32_t)std::atoi(e) : 0u;
    }();
    p.waves_cap = env_waves;
    (void)hipGetLastError();            // launches below report their own errors only
    uint32_t done = 0;                  // frames rendered by the service (the launch path takes the rest)
    if ((rc = serve(c, q, &done)) != VRHIP_OK) return rc;
    if (done == n_frames) return VRHIP_OK;
    if (c->kernel_timing) HIP_TRY(hipEventRecord(c->ev0, c->stream));
    c->ev0_valid = c->kernel_timing;
    while (done < n_frames) {
        const LaunchPlan d = launch_decisions(c, q, p, done);
        if (!d.ovl) c->parity = 0;
        auto& l = c->lane[c->parity];
        hipStream_t rs = d.on_lane ? l.s : c->stream;
        if (d.on_lane && c->join) {         // scene, stream or buffers changed: wait for all of `stream`
            HIP_TRY(hipEventRecord(c->ev_join, c->stream));
            for (auto& ln : c->lane) HIP_TRY(hipStreamWaitEvent(ln.s, c->ev_join, 0));
            c->join = false;
        }
        if (p.use_scratch && (rc = prepare_lane(c, q, d, p, l, rs)) != VRHIP_OK) return rc;
        if ((rc = issue_launch(c, q, d, p, l, rs)) != VRHIP_OK) return rc;
        c->frame += d.k;
        done += d.k;
    }
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    c->timed = true;
    c->flag_synced = false;
    // kernel-time accounting of launches already completed: after this call's
    // launches are queued, so its event queries do not delay them (one frame
    // per synchronous call: they sat between the host's wake-up and the launch)
    if ((rc = account_pending(c, false)) != VRHIP_OK) return rc;
    return VRHIP_OK;
}

int one_render(vrhip_ctx* c, uint32_t n_frames, const uint32_t* times, uint32_t time_seed)
{
    return render_impl(c, n_frames, times, time_seed, 0);
}

int vrhip_render_counted(vrhip_ctx* c, uint32_t n_frames, const uint32_t* times, uint32_t time_seed,
                         uint64_t counters[8])
{
    if (c && !c->group.empty()) return refuse_multi(c, "vrhip_render_counted");
    if (!counters) return fail(VRHIP_ERR_INVALID, "counters is NULL");
    int rc = render_impl(c, n_frames, times, time_seed, 1);
    if (rc) return rc;
    unsigned long long h[vr::kCounters] = {};
    HIP_TRY(hipMemcpyAsync(h, c->counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < vr::kCounters; ++i) counters[i] = (uint64_t)h[i];
    return VRHIP_OK;
}

int vrhip_render_profiled(vrhip_ctx* c, uint32_t n_frames, const uint32_t* times, uint32_t time_seed,
                          uint64_t counters[VRHIP_PROFILE_COUNTERS])
{
    if (c && !c->group.empty()) return refuse_multi(c, "vrhip_render_profiled");
    if (!counters) return fail(VRHIP_ERR_INVALID, "counters is NULL");
    static_assert(VRHIP_PROFILE_COUNTERS == vr::kCounters + vr::kExecCounters, "profile counter layout");
    int rc = render_impl(c, n_frames, times, time_seed, 2);
    if (rc) return rc;
    unsigned long long h[vr::kExecCounterBase + vr::kExecCounters] = {};
    HIP_TRY(hipMemcpyAsync(h, c->counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < vr::kCounters; ++i) counters[i] = (uint64_t)h[i];
    for (int i = 0; i < vr::kExecCounters; ++i) counters[vr::kCounters + i] = (uint64_t)h[vr::kExecCounterBase + i];
    return VRHIP_OK;
}

int vrhip_debug_counters(vrhip_ctx* c, uint64_t out[16], int reset)
{
    if (!c || !out) return fail(VRHIP_ERR_INVALID, "null argument");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    if ((rc = ensure_counters(c)) != VRHIP_OK) return rc;
    unsigned long long h[16] = {};
    HIP_TRY(hipMemcpyAsync(h, c->counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 16; ++i) out[i] = (uint64_t)h[i];
    if (reset) HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(unsigned long long) * kDebugSlots, c->stream));
    return VRHIP_OK;
}

int vrhip_kernel_stats(vrhip_ctx* c, double* total_ms, uint64_t* launches, int reset)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    if ((rc = account_pending(c, true)) != VRHIP_OK) return rc;
    if (total_ms) *total_ms = c->kernel_ms_total;
    if (launches) *launches = c->launches_total;
    if (reset) {
        c->kernel_ms_total = 0.0;
        c->launches_total = 0;
        c->kev_union.clear();
        if (c->kev_origin) { c->kev_free.push_back(c->kev_origin); c->kev_origin = nullptr; }
    }
    return VRHIP_OK;
}

int vrhip_last_launch_info(vrhip_ctx* c, uint32_t* split, uint32_t* use_scratch, uint32_t* kind)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (split) *split = c->last_split;
    if (use_scratch) *use_scratch = c->last_use_scratch;
    if (kind) *kind = c->last_kind;
    return VRHIP_OK;
}

// Waits until the finish pass armed with number `seq` (render_impl) has
// stored it: the host sees the frame complete without the ≈ 13 µs the
// stream's completion signal takes after the kernel (profiles/r06i).  A
// fault or failed launch is caught by the hipStreamQuery made every ≈ 30 µs.
static int wait_flag(vrhip_ctx* c, uint32_t seq)
{
    ++c->sync_flag_waits;
    for (uint32_t n = 1;; ++n) {
        if (__atomic_load_n(c->sync_flag, __ATOMIC_ACQUIRE) == seq) break;
        if ((n & 1023u) == 0u) {
            const hipError_t e = hipStreamQuery(c->stream);
            if (e == hipSuccess) break;                    // drained (the flag is set too)
            if (e != hipErrorNotReady) return fail(VRHIP_ERR_HIP, std::string("sync: ") + hipGetErrorString(e));
        }
        __builtin_ia32_pause();
    }
    c->flag_synced = true;
    return VRHIP_OK;
}

int one_sync(vrhip_ctx* c)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    int rc = set_device(c); if (rc) return rc;
    const uint32_t armed = c->svc.open ? 0u : c->flag_armed;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    if (armed) {
        if ((rc = wait_flag(c, armed)) != VRHIP_OK) return rc;
    } else {
        HIP_TRY(hipStreamSynchronize(c->stream));
        ++c->sync_stream_waits;
    }
    return svc_verify(c);
}

int one_set_sync_flag(vrhip_ctx* c, int on)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    c->sync_flag_mode = on != 0 ? 1 : 0;
    c->flag_armed = 0;
    return VRHIP_OK;
}

int vrhip_sync_info(vrhip_ctx* c, uint64_t out[VRHIP_SYNC_INFO])
{
    if (!c || !out) return fail(VRHIP_ERR_INVALID, "null argument");
    uint64_t a = 0, b = 0;
    for (vrhip_ctx* m : c->group.empty() ? std::vector<vrhip_ctx*>{ c } : c->group) {
        a += m->sync_flag_waits; b += m->sync_stream_waits;
    }
    out[0] = a; out[1] = b;
    return VRHIP_OK;
}

int one_set_overlap(vrhip_ctx* c, int mode)
{
    if (!c || mode < -1 || mode > 1) return fail(VRHIP_ERR_INVALID, "bad overlap mode");
    c->overlap = mode;
    return VRHIP_OK;
}

int one_set_path_split(vrhip_ctx* c, uint32_t groups)
{
    if (!c || groups > 2u * vr::kMaxFramesPerLaunch) return fail(VRHIP_ERR_INVALID, "bad path split");
    c->path_split = groups;
    return VRHIP_OK;
}

int vrhip_last_kernel_ms(vrhip_ctx* c, float* ms)
{
    if (!c || !ms) return fail(VRHIP_ERR_INVALID, "null argument");
    if (set_device(c) == VRHIP_OK) (void)svc_close(c);
    if (!c->timed || !c->ev0_valid) { *ms = 0.f; return VRHIP_OK; }   // no render, or kernel timing off
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return VRHIP_OK;
}

int one_set_kernel_timing(vrhip_ctx* c, int on)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    c->kernel_timing = on != 0;
    return VRHIP_OK;
}
