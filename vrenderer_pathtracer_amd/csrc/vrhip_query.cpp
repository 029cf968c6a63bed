// vrhip_query.cpp -- the queries along the caller's own rays on the device
// (include/vrhip.h): where a ray hits the resident mesh (vrhip_trace_rays,
// vr_rayquery.hip) and what light arrives along it (vrhip_trace_radiance,
// vr_radiance.hip), what the path tracer sees at its first hit
// (vrhip_trace_surface, vr_surface.hip), what light leaves a surface record the
// caller supplies (vrhip_shade_surface, vr_shade.hip), and the current camera's
// rays to feed them (vrhip_camera_rays), and the edge-avoiding filter that turns noisy radiance and the surface
// query's records into an image (vrhip_denoise, vrhip_denoise_frame, vr_denoise.hip),
// and the records that need no ray: at points of the resident mesh
// (vrhip_surface_at) and at the texels of a lightmap atlas of its uvs
// (vrhip_atlas_surface, vr_atlas.hip), and the probe query: radiance from
// points along one shared direction set, projected onto spherical harmonics
// in the call (vrhip_probe_sh, vr_probe.hip), with the irradiance those
// coefficients give at a normal (vrhip_sh_irradiance).  All read the scene
// only: the accumulation, the images and the frame counter stay as they are.
#include <cstddef>
#include <cmath>
#include <cstring>

#include "vr_atlas.hpp"
#include "vr_ctx.hpp"
#include "vr_denoise.hpp"
#include "vr_probe.hpp"
#include "vr_radiance.hpp"
#include "vr_rayquery.hpp"
#include "vr_shade.hpp"
#include "vr_surface.hpp"

// Ray queries against the resident mesh: the path kernels' traversal fed from
// the caller's ray buffer.
static_assert(sizeof(vrhip_ray_hit) == 16 && sizeof(vr::RayHit) == 16, "one 16-B record per ray");
int vrhip_trace_rays(vrhip_ctx* c, const float* d_origins, const float* d_dirs, const float* d_tmax, uint32_t n_rays,
                     uint32_t mode, vrhip_ray_hit* d_hits)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (mode != VRHIP_RAYS_CLOSEST && mode != VRHIP_RAYS_ANY) return fail(VRHIP_ERR_INVALID, "unknown ray query mode");
    if (n_rays > 0 && (!d_origins || !d_dirs || !d_hits)) return fail(VRHIP_ERR_INVALID, "null ray or hit array");
    if (((uintptr_t)d_hits & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_hits is not 16-byte aligned");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_trace_rays");
    if (!c->mesh.loaded()) return fail(VRHIP_ERR_INVALID, "no mesh loaded");
    if (n_rays == 0) return VRHIP_OK;
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    vr::RenderParams p;
    std::memset(&p, 0, sizeof(p));
    mesh_params(c->mesh, p);
    p.verts = nullptr; p.normals = nullptr; p.tangents = nullptr; p.uvs = nullptr;   // a query shades nothing
    p.flags = vr::F_MESH | (c->strict ? (uint32_t)vr::F_STRICT : 0u);
    const vr::RayQuery q{ d_origins, d_dirs, d_tmax, n_rays, mode == VRHIP_RAYS_ANY ? 1u : 0u, c->mesh.a.prim_id,
                          (vr::RayHit*)d_hits };
    const int e = vr::launch_ray_query(p, q, mesh_stack_entries(c->mesh.a.depth), c->cu_count, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("ray query: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

// Radiance along the caller's rays: the whole scene as vrhip_render would
// trace it now (scene_params), the path tracer entered from a ray buffer
// instead of the camera.  The checks come in vrhip_render's order: the
// arguments, nothing to do, the environment, then the device.
static_assert(sizeof(vr::vr4) == 16, "one float4 per ray");
int vrhip_trace_radiance(vrhip_ctx* c, const float* d_origins, const float* d_dirs, const uint32_t* d_seeds,
                         uint32_t n_rays, uint32_t n_samples, float* d_radiance)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (n_rays > 0 && (!d_origins || !d_dirs || !d_seeds || !d_radiance))
        return fail(VRHIP_ERR_INVALID, "null ray, seed or radiance array");
    if (((uintptr_t)d_radiance & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_radiance is not 16-byte aligned");
    if (n_samples < 1u || n_samples > vr::kRadianceMaxSamples)
        return fail(VRHIP_ERR_INVALID, "n_samples is " + std::to_string(n_samples) + " (1 to " +
                                           std::to_string(vr::kRadianceMaxSamples) + ")");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_trace_radiance");
    if (n_rays == 0) return VRHIP_OK;
    if (!c->cornell && !c->hdr)
        return fail(VRHIP_ERR_NO_ENV, "HDRI mode needs an environment map (vrhip_upload_hdr)");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    vr::RenderParams p;
    std::memset(&p, 0, sizeof(p));
    scene_params(c, p);
    const vr::RayRadiance q{ d_origins, d_dirs, d_seeds, n_rays, n_samples, (vr4*)d_radiance };
    (void)hipGetLastError();            // the launch below reports its own error only
    const int e = vr::launch_ray_radiance(p, q, mesh_stack_entries(c->mesh.a.depth), c->cu_count, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("radiance query: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

// Grows the probe scratch to `bytes` (the new buffer before the old one goes,
// as denoise_scratch).
static int probe_scratch(vrhip_ctx* c, size_t bytes)
{
    if (c->probe_bytes >= bytes) return VRHIP_OK;
    void* raw = nullptr;
    if (hipMalloc(&raw, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRHIP_ERR_NOMEM, "probe scratch: " + std::to_string(bytes) + " bytes");
    }
    if (c->probe_scratch) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree((void*)c->probe_scratch);
    }
    c->probe_scratch = (float*)raw; c->probe_bytes = bytes;
    return VRHIP_OK;
}

// Probe radiance on spherical harmonics: vrhip_trace_radiance's scene, session
// handling and order of checks, ray (i, k) = (point i, direction k) traced and
// reduced in one call (include/vrhip.h has the definition).
static_assert(VRHIP_PROBE_BLOCK == (int)vr::kProbeBlock && VRHIP_PROBE_WORDS == (int)vr::kProbeWords,
              "the block and the record of vrhip_probe_sh");
int vrhip_probe_sh(vrhip_ctx* c, const float* d_points, const float* d_dirs, const float* d_weights,
                   const uint32_t* d_probe_seeds, const uint32_t* d_dir_seeds, uint32_t n_probes, uint32_t n_dirs,
                   uint32_t n_samples, float* d_sh)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (n_probes > 0 && (!d_points || !d_dirs || !d_probe_seeds || !d_dir_seeds || !d_sh))
        return fail(VRHIP_ERR_INVALID, "null point, direction, seed or coefficient array");
    if (((uintptr_t)d_sh & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_sh is not 16-byte aligned");
    if (n_samples < 1u || n_samples > vr::kRadianceMaxSamples)
        return fail(VRHIP_ERR_INVALID, "n_samples is " + std::to_string(n_samples) + " (1 to " +
                                           std::to_string(vr::kRadianceMaxSamples) + ")");
    if (n_dirs < 1u || n_dirs > vr::kProbeMaxDirs)
        return fail(VRHIP_ERR_INVALID, "n_dirs is " + std::to_string(n_dirs) + " (1 to " +
                                           std::to_string(vr::kProbeMaxDirs) + ")");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_probe_sh");
    if (n_probes == 0) return VRHIP_OK;
    if (!c->cornell && !c->hdr)
        return fail(VRHIP_ERR_NO_ENV, "HDRI mode needs an environment map (vrhip_upload_hdr)");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    if ((rc = probe_scratch(c, vr::probe_scratch_bytes(n_probes, n_dirs))) != VRHIP_OK) return rc;
    vr::RenderParams p;
    std::memset(&p, 0, sizeof(p));
    scene_params(c, p);
    const vr::ProbeSH q{ d_points, d_dirs, d_weights, d_probe_seeds, d_dir_seeds, n_probes, n_dirs, n_samples,
                         12.566370614f / (float)n_dirs, c->probe_scratch, d_sh };
    (void)hipGetLastError();            // the launches below report their own errors only
    const int e = vr::launch_probe_sh(p, q, mesh_stack_entries(c->mesh.a.depth), c->cu_count, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("probe query: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

// Irradiance at a normal from the records of vrhip_probe_sh: no scene, no mesh.
int vrhip_sh_irradiance(vrhip_ctx* c, const float* d_sh, uint32_t m, const uint32_t* d_index, const float* d_normals,
                        uint32_t n, float* d_out)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (n > 0 && (!d_sh || !d_normals || !d_out)) return fail(VRHIP_ERR_INVALID, "null coefficient, normal or output array");
    if (((uintptr_t)d_out & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_out is not 16-byte aligned");
    if (n > 0 && !d_index && n != m)
        return fail(VRHIP_ERR_INVALID, "no index: n is " + std::to_string(n) + ", m is " + std::to_string(m));
    if (!c->group.empty()) return refuse_multi(c, "vrhip_sh_irradiance");
    if (n == 0) return VRHIP_OK;
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    const vr::SHIrradiance q{ d_sh, m, d_index, d_normals, n, (vr4*)d_out };
    (void)hipGetLastError();            // the launch below reports its own error only
    const int e = vr::launch_sh_irradiance(q, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("sh irradiance: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

// The surface at the first hit of the caller's rays: vrhip_trace_radiance's
// scene, rays and order of checks, intersect_scene and fill_hit run once per
// ray and the record written out.
static_assert(sizeof(vrhip_surface_hit) == 112 && sizeof(vr::SurfaceHit) == 112, "seven 16-B rows per ray");
static_assert(offsetof(vrhip_surface_hit, position) == 16 && offsetof(vrhip_surface_hit, normal) == 32 &&
                  offsetof(vrhip_surface_hit, tangent) == 48 && offsetof(vrhip_surface_hit, color) == 64 &&
                  offsetof(vrhip_surface_hit, specular) == 80 && offsetof(vrhip_surface_hit, emission) == 96,
              "the rows of vrhip_surface_hit");
static_assert(VRHIP_SURF_NONE == (int)vr::kSurfNone && VRHIP_SURF_CORNELL == (int)vr::kSurfCornell &&
                  VRHIP_SURF_SMALL == (int)vr::kSurfSmall && VRHIP_SURF_EXAMPLE == (int)vr::kSurfExample &&
                  VRHIP_SURF_MESH == (int)vr::kSurfMesh, "SurfaceHit::kind");
int vrhip_trace_surface(vrhip_ctx* c, const float* d_origins, const float* d_dirs, uint32_t n_rays,
                        vrhip_surface_hit* d_hits)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (n_rays > 0 && (!d_origins || !d_dirs || !d_hits)) return fail(VRHIP_ERR_INVALID, "null ray or hit array");
    if (((uintptr_t)d_hits & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_hits is not 16-byte aligned");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_trace_surface");
    if (n_rays == 0) return VRHIP_OK;
    if (!c->cornell && !c->hdr)
        return fail(VRHIP_ERR_NO_ENV, "HDRI mode needs an environment map (vrhip_upload_hdr)");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    vr::RenderParams p;
    std::memset(&p, 0, sizeof(p));
    scene_params(c, p);
    const vr::RaySurface q{ d_origins, d_dirs, n_rays, c->mesh.a.prim_id, (vr::SurfaceHit*)d_hits };
    (void)hipGetLastError();            // the launch below reports its own error only
    const int e = vr::launch_ray_surface(p, q, mesh_stack_entries(c->mesh.a.depth), c->cu_count, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("surface query: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

// Radiance from the caller's surface records: vrhip_trace_radiance's scene,
// session handling and order of checks, trace entered at bounce 0's shading
// with the record as its hit.  The kernel reads a record as seven 16-byte
// rows and takes kind and type from the first.
static_assert(offsetof(vrhip_surface_hit, kind) == 4 && offsetof(vrhip_surface_hit, type) == 12 &&
                  offsetof(vr::SurfaceHit, kind) == 4 && offsetof(vr::SurfaceHit, type) == 12 &&
                  offsetof(vr::SurfaceHit, position) == 16 && offsetof(vr::SurfaceHit, normal) == 32 &&
                  offsetof(vr::SurfaceHit, tangent) == 48 && offsetof(vr::SurfaceHit, color) == 64 &&
                  offsetof(vr::SurfaceHit, specular) == 80 && offsetof(vr::SurfaceHit, emission) == 96 &&
                  alignof(vr::SurfaceHit) == 16,
              "the rows surface_shade_kernel loads");
static_assert(vr::kShadeMaxSamples == vr::kRadianceMaxSamples, "one bound on the paths per call");
int vrhip_shade_surface(vrhip_ctx* c, const vrhip_surface_hit* d_hits, const float* d_dirs, const uint32_t* d_seeds,
                        uint32_t n_hits, uint32_t n_samples, float* d_radiance)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (n_hits > 0 && (!d_hits || !d_dirs || !d_seeds || !d_radiance))
        return fail(VRHIP_ERR_INVALID, "null record, direction, seed or radiance array");
    if (((uintptr_t)d_hits & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_hits is not 16-byte aligned");
    if (((uintptr_t)d_radiance & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_radiance is not 16-byte aligned");
    if (n_samples < 1u || n_samples > vr::kShadeMaxSamples)
        return fail(VRHIP_ERR_INVALID, "n_samples is " + std::to_string(n_samples) + " (1 to " +
                                           std::to_string(vr::kShadeMaxSamples) + ")");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_shade_surface");
    if (n_hits == 0) return VRHIP_OK;
    if (!c->cornell && !c->hdr)
        return fail(VRHIP_ERR_NO_ENV, "HDRI mode needs an environment map (vrhip_upload_hdr)");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    vr::RenderParams p;
    std::memset(&p, 0, sizeof(p));
    scene_params(c, p);
    const vr::SurfaceShade q{ (const vr::SurfaceHit*)d_hits, d_dirs, d_seeds, n_hits, n_samples, (vr4*)d_radiance };
    (void)hipGetLastError();            // the launch below reports its own error only
    const int e = vr::launch_surface_shade(p, q, mesh_stack_entries(c->mesh.a.depth), c->cu_count, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("surface shading: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

// The current camera's rays, one per pixel of the whole image, row-major.
int vrhip_camera_rays(vrhip_ctx* c, float* d_origins, float* d_dirs)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (!d_origins || !d_dirs) return fail(VRHIP_ERR_INVALID, "null origin or direction array");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_camera_rays");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    vr::RenderParams p;
    std::memset(&p, 0, sizeof(p));
    camera_params(c, p);
    (void)hipGetLastError();            // the launch below reports its own error only
    const int e = vr::launch_camera_rays(p, d_origins, d_dirs, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("camera rays: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

// The a-trous filter (include/vrhip.h).  The checks on the parameters are
// shared by the two calls and touch no device.
static_assert(sizeof(vrhip_denoise_params) == 20, "five 4-byte words");
static int denoise_params_ok(const vrhip_denoise_params* dp)
{
    if (!dp) return fail(VRHIP_ERR_INVALID, "null denoise params");
    if (dp->n_passes > vr::kDenoiseMaxPasses)
        return fail(VRHIP_ERR_INVALID, "n_passes is " + std::to_string(dp->n_passes) + " (0 to " +
                                           std::to_string(vr::kDenoiseMaxPasses) + ")");
    if (dp->normal_power_log2 > vr::kDenoiseMaxNormalPow)
        return fail(VRHIP_ERR_INVALID, "normal_power_log2 is " + std::to_string(dp->normal_power_log2) + " (0 to " +
                                           std::to_string(vr::kDenoiseMaxNormalPow) + ")");
    if ((dp->flags & ~(uint32_t)VRHIP_DENOISE_DEMODULATE) != 0u) return fail(VRHIP_ERR_INVALID, "unknown denoise flags");
    if (!(std::isfinite(dp->sigma_color) && dp->sigma_color > 0.f))
        return fail(VRHIP_ERR_INVALID, "sigma_color is not finite and greater than 0");
    if (!(std::isfinite(dp->sigma_position) && dp->sigma_position > 0.f))
        return fail(VRHIP_ERR_INVALID, "sigma_position is not finite and greater than 0");
    return VRHIP_OK;
}

// Grows a cached scratch buffer to `cells` cells of `bytes_per_cell`: the new
// one is allocated before the old one goes, so a failure changes nothing.
template <typename T>
static int denoise_scratch(vrhip_ctx* c, T*& buf, size_t& cap, size_t cells, size_t bytes_per_cell)
{
    if (cap >= cells) return VRHIP_OK;
    void* raw = nullptr;
    if (hipMalloc(&raw, cells * bytes_per_cell) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRHIP_ERR_NOMEM, "denoise scratch: " + std::to_string(cells * bytes_per_cell) + " bytes");
    }
    if (buf) {
        (void)hipStreamSynchronize(c->stream);      // the last call's kernels have finished with it (the calls are synchronous)
        (void)hipFree((void*)buf);
    }
    buf = (T*)raw; cap = cells;
    return VRHIP_OK;
}

static vr::Denoise denoise_query(const vrhip_denoise_params* dp, uint32_t w, uint32_t h)
{
    vr::Denoise q{};
    q.w = w; q.h = h;
    q.n_passes = dp->n_passes; q.demodulate = (dp->flags & VRHIP_DENOISE_DEMODULATE) ? 1u : 0u;
    q.normal_pow_log2 = dp->normal_power_log2;
    q.sigma_color = dp->sigma_color; q.sigma_position = dp->sigma_position;
    return q;
}

int vrhip_denoise(vrhip_ctx* c, const float* d_color, const vrhip_surface_hit* d_guides, uint32_t width, uint32_t height,
                  const vrhip_denoise_params* dp, float* d_out)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (!d_color || !d_guides || !d_out) return fail(VRHIP_ERR_INVALID, "null colour, guide or output array");
    if (((uintptr_t)d_color & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_color is not 16-byte aligned");
    if (((uintptr_t)d_guides & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_guides is not 16-byte aligned");
    if (((uintptr_t)d_out & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_out is not 16-byte aligned");
    if (width == 0u || height == 0u || (uint64_t)width * height >= (1ull << 31))
        return fail(VRHIP_ERR_INVALID, "the grid is " + std::to_string(width) + " x " + std::to_string(height) +
                                           " (1 to 2^31 - 1 cells)");
    int rc = denoise_params_ok(dp); if (rc) return rc;
    if (!c->group.empty()) return refuse_multi(c, "vrhip_denoise");
    if ((rc = set_device(c)) != VRHIP_OK) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    const size_t n = (size_t)width * height;
    if ((rc = denoise_scratch(c, c->dn_planes, c->dn_cells, n, vr::kDenoisePlanes * sizeof(vr4))) != VRHIP_OK) return rc;
    vr::Denoise q = denoise_query(dp, width, height);
    q.color = (const vr4*)d_color; q.guides = (const vr::SurfaceHit*)d_guides;
    q.planes = c->dn_planes; q.out = (vr4*)d_out;
    (void)hipGetLastError();            // the launch below reports its own error only
    const int e = vr::launch_denoise(q, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("denoise: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

// The filter on the context's own accumulation: colour = accum * (1 / frames)
// as the tonemap scales it, guides = the surface query on the camera's rays,
// both made in the context's scratch.
int vrhip_denoise_frame(vrhip_ctx* c, const vrhip_denoise_params* dp, float* d_out_f32, uint8_t* d_out_rgba8)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (!d_out_f32 && !d_out_rgba8) return fail(VRHIP_ERR_INVALID, "no output array");
    if (((uintptr_t)d_out_f32 & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_out_f32 is not 16-byte aligned");
    if (((uintptr_t)d_out_rgba8 & 3u) != 0u) return fail(VRHIP_ERR_INVALID, "d_out_rgba8 is not 4-byte aligned");
    int rc = denoise_params_ok(dp); if (rc) return rc;
    if (!c->group.empty()) return refuse_multi(c, "vrhip_denoise_frame");
    if (c->nranks > 1u)
        return fail(VRHIP_ERR_INVALID, "vrhip_denoise_frame: a tiled rank's accumulation holds only its own tiles");
    if ((uint64_t)c->W * c->H >= (1ull << 31)) return fail(VRHIP_ERR_INVALID, "vrhip_denoise_frame: 2^31 pixels or more");
    if (c->frame <= 1u) return fail(VRHIP_ERR_INVALID, "vrhip_denoise_frame: no frame rendered since the last clear");
    if (!c->cornell && !c->hdr)
        return fail(VRHIP_ERR_NO_ENV, "HDRI mode needs an environment map (vrhip_upload_hdr)");
    if ((rc = set_device(c)) != VRHIP_OK) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    const size_t n = (size_t)c->W * c->H;
    if ((rc = denoise_scratch(c, c->dn_planes, c->dn_cells, n, vr::kDenoisePlanes * sizeof(vr4))) != VRHIP_OK) return rc;
    vr::Denoise q = denoise_query(dp, c->W, c->H);
    q.accum = c->accum; q.coef = 1.f / (float)(c->frame - 1u);
    q.planes = c->dn_planes; q.out = (vr4*)d_out_f32; q.out_rgba8 = (vr::u8x4*)d_out_rgba8; q.tone_t = c->tone_t;
    (void)hipGetLastError();            // the launches below report their own errors only
    if (dp->n_passes > 0u) {
        // guides: 112 B a cell, then the rays, 12 + 12 B a cell
        if ((rc = denoise_scratch(c, c->dn_frame, c->dn_frame_cells, n, sizeof(vr::SurfaceHit) + 24u)) != VRHIP_OK) return rc;
        vr::SurfaceHit* guides = (vr::SurfaceHit*)c->dn_frame;
        float* origins = (float*)(c->dn_frame + n * sizeof(vr::SurfaceHit));
        float* dirs = origins + 3u * n;
        vr::RenderParams p;
        std::memset(&p, 0, sizeof(p));
        camera_params(c, p);
        int e = vr::launch_camera_rays(p, origins, dirs, c->stream);
        if (e) return fail(VRHIP_ERR_HIP, std::string("denoise frame, camera rays: ") + hipGetErrorString((hipError_t)e));
        std::memset(&p, 0, sizeof(p));
        scene_params(c, p);
        const vr::RaySurface sq{ origins, dirs, (uint32_t)n, c->mesh.a.prim_id, guides };
        e = vr::launch_ray_surface(p, sq, mesh_stack_entries(c->mesh.a.depth), c->cu_count, c->stream);
        if (e) return fail(VRHIP_ERR_HIP, std::string("denoise frame, guides: ") + hipGetErrorString((hipError_t)e));
        q.guides = guides;
    }
    const int e = vr::launch_denoise(q, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("denoise frame: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

// Grows the atlas scratch to `bytes` (the new buffer before the old one goes,
// as denoise_scratch).
static int atlas_scratch(vrhip_ctx* c, size_t bytes)
{
    if (c->atlas_bytes >= bytes) return VRHIP_OK;
    void* raw = nullptr;
    if (hipMalloc(&raw, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRHIP_ERR_NOMEM, "atlas scratch: " + std::to_string(bytes) + " bytes");
    }
    if (c->atlas_scratch) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree((void*)c->atlas_scratch);
    }
    c->atlas_scratch = (uint8_t*)raw; c->atlas_bytes = bytes;
    return VRHIP_OK;
}

// The record at (prim, u, v) of the resident mesh: vrhip_trace_surface's scene
// and record with no ray.  The inverse of prim_id is built here at first use
// and stays with the mesh (vr_ctx.hpp ResidentMesh).
int vrhip_surface_at(vrhip_ctx* c, const uint32_t* d_prims, const float* d_bary, uint32_t n, vrhip_surface_hit* d_hits)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (n > 0 && (!d_prims || !d_bary || !d_hits)) return fail(VRHIP_ERR_INVALID, "null prim, barycentric or hit array");
    if (((uintptr_t)d_hits & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_hits is not 16-byte aligned");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_surface_at");
    if (!c->mesh.loaded()) return fail(VRHIP_ERR_INVALID, "no mesh loaded");
    if (n == 0) return VRHIP_OK;
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    ResidentMesh& m = c->mesh;
    (void)hipGetLastError();            // the launches below report their own errors only
    if (!m.prim_inv) {
        uint32_t* inv = nullptr;
        if (hipMalloc((void**)&inv, m.n_prims ? (size_t)m.n_prims * sizeof(uint32_t) : 16) != hipSuccess) {
            (void)hipGetLastError();
            return fail(VRHIP_ERR_NOMEM, "prim inverse: " + std::to_string((size_t)m.n_prims * sizeof(uint32_t)) + " bytes");
        }
        const int e = vr::launch_prim_inverse(m.a.prim_id, m.a.n_refs, inv, m.n_prims, c->stream);
        if (e) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipFree(inv);
            return fail(VRHIP_ERR_HIP, std::string("prim inverse: ") + hipGetErrorString((hipError_t)e));
        }
        m.prim_inv = inv;
    }
    vr::RenderParams p;
    std::memset(&p, 0, sizeof(p));
    scene_params(c, p);
    const vr::SurfaceAt q{ d_prims, d_bary, n, m.prim_inv, m.n_prims, (vr::SurfaceHit*)d_hits };
    const int e = vr::launch_surface_at(p, q, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("surface at: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}

// The records of a width x height atlas of the resident mesh's uvs
// (include/vrhip.h has the definition; the kernels: vr_atlas.hip).
int vrhip_atlas_surface(vrhip_ctx* c, uint32_t width, uint32_t height, uint32_t gutter, vrhip_surface_hit* d_hits)
{
    if (!c) return fail(VRHIP_ERR_INVALID, "null ctx");
    if (!d_hits) return fail(VRHIP_ERR_INVALID, "null hit array");
    if (((uintptr_t)d_hits & 15u) != 0u) return fail(VRHIP_ERR_INVALID, "d_hits is not 16-byte aligned");
    if (width == 0u || height == 0u || width > vr::kAtlasMaxSide || height > vr::kAtlasMaxSide ||
        (uint64_t)width * height > vr::kAtlasMaxTexels)
        return fail(VRHIP_ERR_INVALID, "the atlas is " + std::to_string(width) + " x " + std::to_string(height) +
                                           " (1 to 16384 a side, 2^26 texels at most)");
    if (gutter > vr::kAtlasMaxGutter)
        return fail(VRHIP_ERR_INVALID, "gutter is " + std::to_string(gutter) + " (0 to " + std::to_string(vr::kAtlasMaxGutter) + ")");
    if (!c->group.empty()) return refuse_multi(c, "vrhip_atlas_surface");
    if (!c->mesh.loaded()) return fail(VRHIP_ERR_INVALID, "no mesh loaded");
    int rc = set_device(c); if (rc) return rc;
    if ((rc = svc_close(c)) != VRHIP_OK) return rc;
    const uint64_t n = (uint64_t)width * height;
    if ((rc = atlas_scratch(c, vr::atlas_scratch_bytes(n, c->mesh.a.n_refs))) != VRHIP_OK) return rc;
    vr::RenderParams p;
    std::memset(&p, 0, sizeof(p));
    scene_params(c, p);
    const vr::Atlas q{ width, height, gutter, c->mesh.a.prim_id, c->atlas_scratch, (vr::SurfaceHit*)d_hits };
    (void)hipGetLastError();            // the launches below report their own errors only
    const int e = vr::launch_atlas_surface(p, q, c->cu_count, c->stream);
    if (e) return fail(VRHIP_ERR_HIP, std::string("atlas surface: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return svc_verify(c);
}
