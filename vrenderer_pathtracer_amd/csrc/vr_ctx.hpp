// vr_ctx.hpp -- internal to the host half of libvrhip.so (vrhip_scene, _mesh, _query, _service, _render, _multi
// and _selftest.cpp, which implement include/vrhip.h): the context, the resident mesh it owns, the error
// helpers and the functions one unit calls in another.  The host half is the device-side counterpart of
// vRendererCuda (src/vRendererCuda.cpp) and the cu_* device ABI (cuda/include/PathTracer.cuh:107-165), re-designed
// around one context per GPU, status codes instead of exit(0) (src/vRendererCuda.cpp:454-467), flags
// passed by value in the launch instead of __constant__ symbol copies (cuda/src/PathTracer.cu:976-1001),
// and multi-frame render steps.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cstdint>
#include <deque>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vrhip.h"
#include "vr_devmesh.hpp"
#include "vr_params.hpp"

using vr::vr3;
using vr::vr2;
using vr::vr4;

// nothing below is part of the library's surface
#pragma GCC visibility push(hidden)

// records msg for vrhip_last_error (per thread) and returns code
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(VRHIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

template <typename T>
void dfree(T*& p) { if (p) { (void)hipFree((void*)p); p = nullptr; } }

// a device temporary that is freed on every way out of its scope
struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
template <typename T>
using dev_ptr = std::unique_ptr<T, DevFree>;
template <typename T>
hipError_t dev_alloc(dev_ptr<T>& p, size_t bytes)
{
    void* raw = nullptr;
    const hipError_t e = hipMalloc(&raw, bytes);
    p.reset((T*)raw);
    return e;
}

// The resident triangle mesh and the one place that frees it: the arrays the
// kernels, the builders, the refit and the ray query share (vr_devmesh.hpp
// MeshArrays: pointers, compact nodes and triangles, depth) and what only the
// host keeps.  An upload fills a fresh one and swaps it with the context's
// when nothing failed, so a refused mesh leaves the resident one as it was;
// the old arrays go when the fresh one's scope ends.  A loaded mesh has at
// least one node.
struct ResidentMesh {
    vr::MeshArrays a{};
    // a device build's status record, reused for the refit's validation flags;
    // with a.slot_vert and a.node_level what vrhip_refit_mesh_device needs
    // (all three null after a host upload, which keeps no index data)
    vr::DevBuildStatus* status = nullptr;
    size_t n_bvh = 0, n_slots = 0;                // the reference layout's float4 rows and slots
    uint32_t bvh_nodes = 0;                       // its node count (vrhip_bvh_info)
    uint32_t refit_verts = 0;                     // the device upload's n_verts
    // what prim_id's values range over: the caller's triangles after a device
    // build, the flat slots after a host upload
    uint32_t n_prims = 0;
    // the inverse of a.prim_id, u32[n_prims]: the lowest compact triangle of each
    // prim (vr_atlas.hpp launch_prim_inverse).  Built at the first
    // vrhip_surface_at, gone with the mesh at the next upload; a refit moves no
    // triangle and keeps it.
    uint32_t* prim_inv = nullptr;

    ResidentMesh() = default;
    ResidentMesh(const ResidentMesh&) = delete;
    ResidentMesh& operator=(const ResidentMesh&) = delete;
    ResidentMesh(ResidentMesh&& o) noexcept { swap(o); }
    ResidentMesh& operator=(ResidentMesh&& o) noexcept { swap(o); return *this; }
    ~ResidentMesh()
    {
        dfree(a.bvh); dfree(a.bvh16); dfree(a.verts); dfree(a.tri_e); dfree(a.tpath); dfree(a.normals);
        dfree(a.tangents); dfree(a.uvs); dfree(a.slot_vert); dfree(a.node_level); dfree(a.prim_id); dfree(status);
        dfree(prim_inv);
    }
    bool loaded() const { return a.bvh != nullptr; }
    void swap(ResidentMesh& o)
    {
        std::swap(a, o.a); std::swap(status, o.status); std::swap(n_bvh, o.n_bvh); std::swap(n_slots, o.n_slots);
        std::swap(bvh_nodes, o.bvh_nodes); std::swap(refit_verts, o.refit_verts);
        std::swap(n_prims, o.n_prims); std::swap(prim_inv, o.prim_inv);
    }
    // arrays for max_nodes nodes and n_refs compact triangles (every array at
    // least 16 bytes) into an empty mesh; with_refit_data: slot_vert,
    // node_level and the status record too.  The shape fields stay the caller's.
    int alloc(uint32_t max_nodes, uint32_t n_refs, bool with_refit_data)
    {
        auto get = [](auto*& p, size_t bytes) {
            const hipError_t e = hipMalloc((void**)&p, bytes ? bytes : 16);
            if (e != hipSuccess) (void)hipGetLastError();    // reported here: later launches check hipGetLastError
            return e;
        };
        const size_t nv = 3 * (size_t)n_refs;
        HIP_TRY(get(a.bvh, 4 * (size_t)max_nodes * 16));
        HIP_TRY(get(a.bvh16, 2 * (size_t)max_nodes * 16));
        HIP_TRY(get(a.verts, nv * sizeof(vr3)));
        HIP_TRY(get(a.tri_e, nv * sizeof(vr3)));
        HIP_TRY(get(a.tpath, (size_t)n_refs * sizeof(unsigned long long)));
        HIP_TRY(get(a.normals, nv * 16));
        HIP_TRY(get(a.tangents, nv * 16));
        HIP_TRY(get(a.uvs, nv * 8));
        HIP_TRY(get(a.prim_id, (size_t)n_refs * sizeof(uint32_t)));
        if (!with_refit_data) return VRHIP_OK;
        HIP_TRY(get(a.slot_vert, nv * sizeof(uint32_t)));
        HIP_TRY(get(a.node_level, (size_t)max_nodes * sizeof(uint32_t)));
        HIP_TRY(get(status, sizeof(vr::DevBuildStatus)));
        return VRHIP_OK;
    }
};

// Path streams (see render_impl): launch i's kernels wait for the finish
// pass of launch i - VR_PATH_STREAMS, the last reader of the same scratch.
#ifndef VR_PATH_STREAMS
#define VR_PATH_STREAMS 3
#endif

struct vrhip_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    uint32_t W = 0, H = 0;
    vr4* accum = nullptr;
    float* cam_sxy = nullptr;                   // camera-ray screen offsets: W column values, then H row values
    vr::u8x4* rgba = nullptr;
    vr::u8x4* depth = nullptr;
    // camera (vCamera, cuda/include/PathTracer.cuh:58-84)
    float cam_o[3] = { 0.f, 0.f, 150.f }, cam_d[3] = { 0.f, 0.f, -1.f };
    float cam_up[3] = { 0.f, 1.f, 0.f }, cam_right[3] = { 1.f, 0.f, 0.f };
    float fov_scale = 0.f;
    uint32_t frame = 1;                         // m_frame (src/vRendererCuda.cpp:24)
    float fresnel_coef = 0.1f, fresnel_pow = 3.f; // src/vRendererCuda.cpp:27-28
    bool cornell = false, example = false, view_brdf = false;
    bool strict = false;          // exact reference traversal (no t-culling)
    ResidentMesh mesh;            // the triangle mesh (vrhip_mesh.cpp)
    // environment / textures / brdf
    vr4* hdr = nullptr; uint32_t hdr_w = 0, hdr_h = 0;
    vr4* tex[3] = { nullptr, nullptr, nullptr }; uint32_t tex_w[3] = { 0, 0, 0 }, tex_h[3] = { 0, 0, 0 };
    float* brdf = nullptr;
    // sharding
    uint32_t rank = 0, nranks = 1;
    // path groups per pixel (0: automatic) and their result scratch
    uint32_t path_split = 0;
    uint32_t cu_count = 256;
    // Render launches take the path streams in turn, each with its own
    // scratch, so a launch's paths can start while the previous launch
    // drains; finish passes stay in order on `stream` (see render_impl)
    struct Lane {
        hipStream_t s = nullptr;
        vr4* paths = nullptr;
        size_t paths_cap = 0;        // float4 elements
        vr4* prim = nullptr;         // primary hits, 2 float4 per owned pixel
        size_t prim_cap = 0;         // float4 elements
        uint32_t* chunk_ctr = nullptr;   // wave kernel work queue heads
        // longest-first scheduling: per sub-tile costs measured by a launch
        // on this scratch and the per-XCD order sorted from them, in two
        // slots used by turns (ordered launch i measures into slot oi and
        // takes the order launch i-2 left there: its sort is long finished,
        // so the launch waits for nothing -- with one slot, a one-frame
        // call's launch waited for the sort of the call before, ≈ 12 µs of
        // cross-stream hand-off per synchronous frame, r05)
        uint32_t* sub_cost[2] = { nullptr, nullptr };
        uint32_t* sub_order[2] = { nullptr, nullptr };
        size_t sub_cap = 0;          // sub-tiles the buffers hold
        uint32_t order_nsub[2] = { 0, 0 };   // sub-tile count each slot's order was sorted for (0: none)
        uint32_t oi = 0;             // the slot the next ordered launch uses
        uint32_t* px_list = nullptr;     // F_SPARSE launches: the pixels whose camera ray hits (RenderParams::sparse_px)
        size_t px_cap = 0;
        hipEvent_t done = nullptr;   // recorded on `s` after the render kernels
        hipEvent_t finished = nullptr;   // recorded on `stream` after the finish pass that read this scratch
        hipEvent_t ordered[2] = { nullptr, nullptr };   // recorded on `s` after the order pass of each slot
        bool order_pending[2] = { false, false };       // an order pass was queued on the slot since a launch waited for it
        bool used = false;
    } lane[VR_PATH_STREAMS];
    uint32_t parity = 0;
    int overlap = -1;            // vrhip_set_overlap: 1 always, 0 never, -1 small launches only
    bool cost_order = true;      // longest-first sub-tile order for small launches (VRHIP_COST_ORDER=0: off)
    bool join = true;            // the next launches must wait for everything queued on `stream`
    hipEvent_t ev_join = nullptr;
    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // render-kernel start/stop event pairs not yet added to the totals (read
    // without blocking at the next render, all of them by vrhip_kernel_stats),
    // and recycled events
    struct Span { hipEvent_t first, second; uint32_t launches; };
    std::deque<Span> kev_pending;
    std::vector<hipEvent_t> kev_free;
    bool timed = false;          // ev1 marks the end of the last render
    bool ev0_valid = false;      // ev0 marks its start (kernel timing on)
    // vrhip_set_kernel_timing (VRHIP_KERNEL_TIMING=0: off): span events around
    // every launch's render kernels (vrhip_kernel_stats) and each call
    // (vrhip_last_kernel_ms)
    bool kernel_timing = true;
    float* tone_t = nullptr;     // the tonemap threshold table (vr_kernel.hpp tone_byte), filled at creation
    double kernel_ms_total = 0.0;    // union of the launches' render-kernel spans (overlapping launches count once)
    uint64_t launches_total = 0;
    uint32_t last_split = 1, last_use_scratch = 0, last_kind = 0;   // vrhip_last_launch_info
    // spans as [start, end) in ms after kev_origin (the start event of the
    // first span since the last reset), merged into disjoint intervals: launches
    // on different path streams can start out of queue order
    hipEvent_t kev_origin = nullptr;
    std::vector<std::pair<double, double>> kev_union;
    unsigned long long* counters = nullptr;
    // vrhip_denoise / vrhip_denoise_frame scratch, grown on demand and kept
    // (vrhip_query.cpp): the filter's four float4 planes, and the frame call's
    // guide records, colour plane and camera rays
    vr4* dn_planes = nullptr; size_t dn_cells = 0;
    uint8_t* dn_frame = nullptr; size_t dn_frame_cells = 0;
    // vrhip_atlas_surface scratch, grown on demand and kept: the cell planes
    // and the queue of large triangles (vr_atlas.hpp atlas_scratch_bytes)
    uint8_t* atlas_scratch = nullptr; size_t atlas_bytes = 0;
    // vrhip_probe_sh scratch, grown on demand and kept: the block partials of
    // a call with more than 64 directions (vr_probe.hpp probe_scratch_bytes)
    float* probe_scratch = nullptr; size_t probe_bytes = 0;
    // GL interop (colour, depth textures registered by the display host)
    hipGraphicsResource_t gl_res[2] = { nullptr, nullptr };
    // render service (vrhip_set_service): a session of launches on one
    // persistent kernel (vr_kernel.hpp service_body), see svc_open
    struct Session {
        bool open = false;
        hipStream_t s = nullptr;                  // the service stream
        // descriptor rings in host-pinned coherent memory, one per session in
        // turn: a closed session's kernel may still read its ring while the
        // next session fills the other (ring_done: after that kernel)
        vr::SvcHostCtl* rings[2] = { nullptr, nullptr };
        vr::SvcHostCtl* rings_dev[2] = { nullptr, nullptr };
        hipEvent_t ring_done[2] = { nullptr, nullptr };
        bool ring_used[2] = { false, false };
        uint32_t ring_i = 0;
        uint32_t cur_ring = 0;                    // the open (or last) session's ring
        // per ring: the launches its last session summed, and whether the
        // kernel's count of consumed launches (SvcHostCtl::retired) was checked
        uint32_t ring_posted[2] = { 0, 0 };
        bool ring_checked[2] = { true, true };
        vr::SvcHostCtl* host = nullptr;           // the open session's ring
        vr::SvcDevCtl* dev = nullptr;             // device mirror of the ring
        uint32_t* qctl = nullptr; size_t qctl_slots = 0;    // work-queue heads per launch slot
        uint8_t* scratch = nullptr; size_t scratch_cap = 0; // launch slots' path results
        vr4* prim = nullptr; size_t prim_cap = 0;           // the session's primary records, 2 float4 per owned pixel
        uint32_t* subs = nullptr; size_t subs_cap = 0;      // F_SPARSE sessions: the pixels whose camera ray hits
        uint8_t* staging = nullptr; size_t staging_cap = 0; // deferred gathers: per launch slot
        uint32_t slots = 0, kmax = 0, posted = 0;
        size_t slot_bytes = 0;
        int stack = 16;
        uint32_t n_tiles = 0;
        vr::RenderParams p{};                     // the session's launch parameters
        vr::RenderParams key{};                   // what must not change within a session (svc_key)
        vr::SvcFinish fin{};
        std::vector<std::pair<uint32_t, int>> gathers;   // deferred vrhip_comm_gather: (launch, what)
        std::chrono::steady_clock::time_point last_post;
        hipEvent_t k0 = nullptr, k1 = nullptr;    // the service kernel's span
        hipEvent_t finished = nullptr;            // recorded on `stream` after the session's finish pass
        bool finished_used = false;
        // recorded on `stream` right after the finish pass, before the
        // session's deferred gathers; the next session's kernel waits for it
        // instead of for everything on `stream` when nothing it reads was
        // queued there since (stream_epoch unchanged), so it overlaps them
        hipEvent_t summed = nullptr;
        uint64_t summed_epoch = 0;
        bool summed_valid = false;
    } svc;
    // bumped by everything that queues work the render kernels read on
    // `stream` (uploads and other quiesce() callers, clears): Session::summed
    uint64_t stream_epoch = 0;
    int service = -1;                             // 1 every production mesh launch, 0 never, -1 automatic
    // vrhip_set_service_timing (test hook; 0 = default): the kernel's idle
    // limit, the host's post window, a host delay between the window check
    // and the post (forces the retire-vs-post race)
    uint32_t svc_idle_us = 0, svc_window_us = 0, svc_post_delay_us = 0;
    uint64_t svc_refused = 0;                     // launches a retiring session kernel did not take
    // vrhip_service_info: sessions opened, launches they took, gathers deferred
    // to a session's close, sessions the scratch allocation could not open
    uint64_t svc_sessions = 0, svc_served = 0, svc_deferred = 0, svc_alloc_fallbacks = 0;
    size_t svc_budget = 0;                        // vrhip_set_service_budget (0: VRHIP_SERVICE_BYTES / 24 GiB)
    // multi-device renderer (vrhip_create_multi): the lead context holds every
    // member context (itself first); settings fan out to all of them
    std::vector<vrhip_ctx*> group;
    // one-frame launches as a HIP graph (VRHIP_GRAPH=1; one_frame_graph): the
    // path kernel + finish pass captured once per longest-first order slot,
    // their kernel arguments updated per frame
    struct FrameGraph {
        hipGraph_t g = nullptr;
        hipGraphExec_t x = nullptr;
        hipGraphNode_t kn[2] = { nullptr, nullptr };
        hipKernelNodeParams kp[2] = {};
        vr::RenderParams key{};               // the launch parameters except the frame's number and seed
        vr::RenderParams arg{};               // this frame's parameters (the nodes' argument)
        bool valid = false;
    } fgraph[2];
    bool use_graph = false;
    uint64_t graph_launches = 0, graph_captures = 0;
    // completion flag of a synchronous one-frame call (VRHIP_SYNC_FLAG): the
    // finish pass's last block stores the call's number to host-coherent
    // memory, and vrhip_sync polls it instead of waiting for the stream's
    // completion signal (vr_kernel.hip finish_arrive)
    int sync_flag_mode = 1;
    uint32_t* sync_flag = nullptr;   // host-coherent
    uint32_t* sync_ctr = nullptr;    // device: the finish pass's block arrivals
    uint32_t sync_seq = 0;
    uint32_t flag_armed = 0;         // the number the last queued work ends with (0: none)
    bool flag_synced = false;        // the last sync saw it: no render in flight
    bool stream_shared = false;      // the caller has the stream (vrhip_get/set_stream): no flag
    uint64_t sync_flag_waits = 0, sync_stream_waits = 0;
    // the lead of a group: renders since the colour / depth tiles were last
    // gathered (the gather runs when the lead's images are next needed)
    bool group_stale = false;
    // multi-GPU tile gather (vrhip_comm_*): one RCCL communicator per context
    ncclComm_t comm = nullptr;
    uint8_t* comm_send = nullptr;    // this rank's packed tiles (largest element, 16 B/pixel)
    uint8_t* comm_recv = nullptr;    // rank 0: n_ranks packed buffers, comm_slot bytes apart
    size_t comm_slot = 0;            // bytes per rank slot (max owned pixels x 16 B)
    uint32_t comm_rank = 0, comm_n = 0;   // the communicator's rank and size (tiling fixed while it exists)
};

// vrhip_service.cpp
void svc_free(vrhip_ctx* c);
int svc_close(vrhip_ctx* c);
int svc_verify(vrhip_ctx* c);
uint32_t svc_slots(const vrhip_ctx* c, uint32_t path_stride, uint32_t kmax, size_t* slot_bytes_out);
int svc_open(vrhip_ctx* c, const vr::RenderParams& p, int stack, uint32_t n_tiles, uint32_t kmax);
bool svc_post(vrhip_ctx* c, uint32_t k, const uint32_t* times, uint32_t time_seed);
bool svc_fits(const vrhip_ctx* c, const vr::RenderParams& p, uint32_t k);
int one_set_service(vrhip_ctx* c, int mode);
// vrhip_render.cpp
int take_event(vrhip_ctx* c, hipEvent_t* e);
int one_render(vrhip_ctx* c, uint32_t n_frames, const uint32_t* times, uint32_t time_seed);
int one_sync(vrhip_ctx* c);
int one_set_sync_flag(vrhip_ctx* c, int on);
int one_set_overlap(vrhip_ctx* c, int mode);
int one_set_path_split(vrhip_ctx* c, uint32_t groups);
int one_set_kernel_timing(vrhip_ctx* c, int on);
// vrhip_scene.cpp
int one_set_camera(vrhip_ctx* c, const float origin[3], const float dir[3], const float up[3],
                   const float right[3], float fov_scale);
int one_clear(vrhip_ctx* c);
int one_set_fresnel(vrhip_ctx* c, float coef, float power);
int one_use_cornell_box(vrhip_ctx* c, int e);
int one_use_example_sphere(vrhip_ctx* c, int e);
int one_set_strict_traversal(vrhip_ctx* c, int e);
int one_use_brdf(vrhip_ctx* c, int e);
int one_upload_hdr(vrhip_ctx* c, const float* rgba, uint32_t w, uint32_t h);
int one_upload_hdr_half(vrhip_ctx* c, const uint16_t* rgba_half, uint32_t w, uint32_t h);
int one_upload_texture(vrhip_ctx* c, int type, const float* rgba, uint32_t w, uint32_t h);
int one_upload_brdf(vrhip_ctx* c, const float* table, size_t n_floats);
// the device layout of a planar R,G,B MERL table of 3*1458000 floats: entry i's three channels adjacent
std::vector<float> brdf_interleaved(const float* table);
// vrhip_multi.cpp
int refuse_multi(vrhip_ctx* c, const char* what);
int multi_gather(vrhip_ctx* c, int what);
int multi_images(vrhip_ctx* c);

inline int set_device(vrhip_ctx* c) { HIP_TRY(hipSetDevice(c->device)); return VRHIP_OK; }

// The mesh fields of a launch's parameters; all zero when nothing is loaded.
inline void mesh_params(const ResidentMesh& m, vr::RenderParams& p)
{
    const vr::MeshArrays& a = m.a;
    p.bvh = a.bvh; p.bvh16 = a.bvh16; p.verts = a.verts; p.tri_e = a.tri_e; p.tpath = a.tpath;
    p.normals = a.normals; p.tangents = a.tangents; p.uvs = a.uvs;
    p.n_nodes = a.n_nodes; p.n_tris = a.n_refs;
}

// The scene half of a launch's parameters, what a path reads once it has its
// ray: the flag word, the mesh, the environment, the texture maps, the BRDF
// table and the Fresnel parameters.  vrhip_render (build_params) and
// vrhip_trace_radiance trace the same scene through it.
inline void scene_params(const vrhip_ctx* c, vr::RenderParams& p)
{
    p.fresnel_coef = c->fresnel_coef; p.fresnel_pow = c->fresnel_pow;
    uint32_t f = 0;
    if (c->cornell) f |= vr::F_CORNELL;
    if (c->example) f |= vr::F_EXAMPLE;
    if (c->view_brdf) f |= vr::F_VIEW_BRDF;
    if (c->strict) f |= vr::F_STRICT;
    // the reference skips the mesh while the example sphere is on
    // (PathTracer.cu:192,268): a sphere scene, whatever mesh is loaded
    if (c->mesh.loaded() && !c->example) f |= vr::F_MESH;
    if (c->brdf) f |= vr::F_BRDF;
    if (c->tex[0]) f |= vr::F_TEX_DIFF;
    if (c->tex[1]) f |= vr::F_TEX_NORM;
    if (c->tex[2]) f |= vr::F_TEX_SPEC;
    p.flags = f;
    mesh_params(c->mesh, p);
    p.hdr = c->hdr; p.hdr_w = c->hdr_w; p.hdr_h = c->hdr_h;
    for (int i = 0; i < 3; ++i) { p.tex[i] = c->tex[i]; p.tex_w[i] = c->tex_w[i]; p.tex_h[i] = c->tex_h[i]; }
    p.brdf = c->brdf;
}

// The camera half of a launch's parameters: what camera_ray reads.
// vrhip_render (build_params) and vrhip_camera_rays take the same camera
// through it.
inline void camera_params(const vrhip_ctx* c, vr::RenderParams& p)
{
    p.cam_o = vr4{ c->cam_o[0], c->cam_o[1], c->cam_o[2], 0.f };
    p.cam_d = vr4{ c->cam_d[0], c->cam_d[1], c->cam_d[2], 0.f };
    // PathTracer.cu:833-836 in the same fp32 operation order
    const float sx = c->fov_scale * (float)c->W / (float)c->H;
    p.cx = vr4{ sx * c->cam_right[0], sx * c->cam_right[1], sx * c->cam_right[2], 0.f };
    p.cy = vr4{ c->fov_scale * c->cam_up[0], c->fov_scale * c->cam_up[1], c->fov_scale * c->cam_up[2], 0.f };
    p.W = c->W; p.H = c->H;
    p.cam_sxy = c->cam_sxy;
}

// traversal stack entries for a tree of this depth (the walk needs depth + 1),
// rounded up to a size the kernels are built for
inline int mesh_stack_entries(uint32_t depth) { return depth <= 15 ? 16 : depth <= 23 ? 24 : depth <= 30 ? 32 : 64; }

inline uint32_t rendered_rows(const vrhip_ctx* c) { return (c->H / 16u) * 16u; }

// 16x16 tiles of the rendered region, dealt round-robin: rank r owns tiles
// r, r + n, r + 2n, ... (row-major tile order)
inline uint32_t owned_tiles_of(uint32_t W, uint32_t H, uint32_t rank, uint32_t n_ranks)
{
    const uint32_t total = (W / 16u) * (H / 16u);
    return total > rank ? (total - rank + n_ranks - 1u) / n_ranks : 0u;
}

// Waits for the path streams' render kernels (they read the scene and their
// scratch) and makes the next launches wait for all work queued on `stream`.
// Every call that replaces device buffers or the stream goes through here.
inline void quiesce(vrhip_ctx* c)
{
    (void)svc_close(c);
    ++c->stream_epoch;
    if (c->svc.s) (void)hipStreamSynchronize(c->svc.s);
    for (auto& l : c->lane)
        if (l.s) (void)hipStreamSynchronize(l.s);
    c->join = true;
}

#pragma GCC visibility pop
