// vrhip_query.cpp -- the queries along the caller's own rays on the device
// (include/vrhip.h): where a ray hits the resident mesh (vrhip_trace_rays,
// vr_rayquery.hip) and what light arrives along it (vrhip_trace_radiance,
// vr_radiance.hip), what the path tracer sees at its first hit
// (vrhip_trace_surface, vr_surface.hip), what light leaves a surface record the
// caller supplies (vrhip_shade_surface, vr_shade.hip), and the current camera's
// rays to feed them (vrhip_camera_rays).  All read the scene only: the accumulation, the
// images and the frame counter stay as they are.
#include <cstddef>
#include <cstring>

#include "vr_ctx.hpp"
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
