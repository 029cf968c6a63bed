/*
 * vrhip.h -- C ABI of libvrhip.so, the MI355X (gfx950) path-tracing backend
 * that drops in behind the reference's vRenderer interface as vRendererHIP.
 *
 * Plain C: opaque handle, plain pointers and sizes, int status codes
 * (0 = VRHIP_OK, never exit()).  All host pointers are copied; the library
 * never frees caller memory.  Calls on one context are not re-entrant (the
 * reference runs everything on the Qt GUI thread, src/NGLScene.cpp:249-472).
 *
 * Each entry point names the reference interface it replaces.  Reference
 * paths are relative to the v0q/vRenderer_PathTracer repository root.
 */
#ifndef VRHIP_H
#define VRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRHIP_ABI_VERSION 6

typedef enum vrhip_status {
    VRHIP_OK = 0,
    VRHIP_ERR_INVALID = -1,      /* bad argument / handle */
    VRHIP_ERR_HIP = -2,          /* HIP runtime error (see vrhip_last_error) */
    VRHIP_ERR_NO_ENV = -3,       /* HDRI mode with no environment loaded */
    VRHIP_ERR_BVH = -4,          /* malformed or too-deep flattened BVH */
    VRHIP_ERR_NO_DEVICE = -5,
    VRHIP_ERR_NOMEM = -6,
    VRHIP_ERR_COMM = -7          /* RCCL error (see vrhip_last_error) */
} vrhip_status;

/* vTextureType, cuda/include/PathTracer.cuh:86 */
typedef enum vrhip_texture_type { VRHIP_TEX_DIFFUSE = 0, VRHIP_TEX_NORMAL = 1, VRHIP_TEX_SPECULAR = 2 } vrhip_texture_type;

typedef struct vrhip_ctx vrhip_ctx;

/* Thread-local text of the last error. */
const char *vrhip_last_error(void);
int vrhip_abi_version(void);
/* SHA-256 (hex) of the sources, this header and the compile flags the
 * library was built from; the Python loader rebuilds when it differs from
 * the files on disk, and bench.py / smoke() print it. */
const char *vrhip_build_id(void);
int vrhip_device_count(int *count);

/* ---- lifetime -------------------------------------------------------- */
/* replaces vRendererCuda::init (src/vRendererCuda.cpp:38-55): allocates the
 * float4[W*H] accumulation buffer and the RGBA8 colour/depth images on
 * `device`, zero-fills, frame counter = 1.  1 <= width, height <= 65535. */
int vrhip_create(int device, uint32_t width, uint32_t height, vrhip_ctx **out);
/* One renderer over several GPUs of this process (SURVEY 8(b) "create_multi";
 * no reference counterpart: the reference's caller creates one renderer,
 * src/NGLScene.cpp:82-89).  A member context per device in `devices` (no
 * repeats), member i rendering the 16x16 tiles vrhip_set_tiling deals rank i
 * of n; the
 * RCCL communicators are made in one call (ncclCommInitAll).  The returned
 * context is the lead (devices[0]): every setting and upload on it fans out
 * to all members; vrhip_render renders every device's tiles (each member
 * with its own render service for back-to-back calls, vrhip_set_service), and
 * the RGBA8 and depth tiles are gathered to the lead (one grouped ncclGather
 * each) when the lead's images are next needed -- vrhip_read_rgba8/depth8,
 * vrhip_gl_present, vrhip_device_buffers, vrhip_sync -- so read-back and GL
 * presentation show the whole frame; vrhip_read_accum gathers the
 * accumulation first; vrhip_comm_gather gathers the given image.  Refused on
 * it: vrhip_set_tiling, vrhip_set_stream, vrhip_comm_init/destroy, the
 * service test hooks, the counting renders.  n = 1 is allowed (the same code,
 * a one-rank communicator). */
int vrhip_create_multi(const int *devices, uint32_t n_devices, uint32_t width, uint32_t height, vrhip_ctx **out);
/* The devices of a context (one for vrhip_create, the group for
 * vrhip_create_multi, lead first); `devices` may be NULL (count only). */
int vrhip_device_group(vrhip_ctx *ctx, uint32_t *n_devices, int *devices);
/* replaces vRendererCuda::cleanUp + cu_cleanUp (src/vRendererCuda.cpp:167-199,
 * cuda/src/PathTracer.cu:1009-1030). NULL is a no-op. */
int vrhip_destroy(vrhip_ctx *ctx);
/* Run subsequent work on this hipStream_t (NULL = the context's own stream). */
int vrhip_set_stream(vrhip_ctx *ctx, void *hip_stream);
void *vrhip_get_stream(vrhip_ctx *ctx);
/* Streams.  A context has one "context stream": its own (created
 * non-blocking with the context, so it does not synchronise with the NULL
 * stream) or the one vrhip_set_stream gave it; vrhip_get_stream returns it.
 * vrhip_set_stream waits for the stream it leaves, so work does not reorder
 * across the change; it is refused on a multi-device context.
 *   Where the work runs.  Uploads, clears, the device mesh builds and the
 * refit, every query (vrhip_trace_rays/radiance/surface, vrhip_shade_surface,
 * vrhip_probe_sh, vrhip_sh_irradiance, vrhip_surface_at, vrhip_atlas_surface,
 * vrhip_camera_rays, vrhip_denoise, vrhip_denoise_frame), the read-backs,
 * vrhip_pack_tiles/unpack_tiles and vrhip_comm_gather are queued on the
 * context stream in call order.  vrhip_render's path kernels run there too
 * or on internal streams (the path streams, the render service's), ordered
 * by events against the context stream; what writes the accumulation and the
 * images -- the finish pass, or a sphere scene's render kernel -- always runs
 * on the context stream.
 *   Device inputs (the d_ arguments of the device uploads, the refit and the
 * queries) must be complete, or pending on the context stream: work queued
 * there before the call -- the kernel that still produces the rays, a copy --
 * is ordered ahead of the library's reads.  Work on any OTHER stream, the NULL
 * stream included, is not waited for: synchronise it or make the context
 * stream wait for its event first.
 *   After vrhip_render, a caller that holds the context stream or the buffers
 * (vrhip_set_stream, vrhip_get_stream, vrhip_device_buffers, taken BEFORE the
 * render) may queue its own work on the context stream -- a copy out of the
 * buffers, a collective -- with no library call in between, and that work
 * sees every frame of the renders before it:
 *   service mode -1 (automatic, the default) and 0: always.  Such a context
 *     never joins a render service session on its own, because a session's
 *     images arrive with the finish pass that its close enqueues.
 *   service mode 1 (explicit): after the next call that closes the session
 *     (the list is at vrhip_set_service; vrhip_device_buffers is one).  The
 *     close waits for nothing on the host: it enqueues the finish pass on the
 *     context stream, so work queued there behind the closing call sees the
 *     session's frames.
 * vrhip_sync on such a context waits for the whole context stream, the
 * caller's own work on it included. */

/* ---- per-frame state -------------------------------------------------- */
/* replaces vRendererCuda::updateCamera (src/vRendererCuda.cpp:69-98): copies
 * the camera (xyz used, w = 0 as in the reference), resets frame = 1 and
 * clears the accumulation buffer. */
int vrhip_set_camera(vrhip_ctx *ctx, const float origin[3], const float dir[3],
                     const float up[3], const float right[3], float fov_scale);
/* replaces vRendererCuda::clearBuffer (src/vRendererCuda.cpp:100-105) and
 * cu_fillFloat4 (cuda/src/PathTracer.cu:1003-1007). */
int vrhip_clear(vrhip_ctx *ctx);
/* Stores the Fresnel parameters passed by value to every launch
 * (include/vRenderer.h:139-145; the base class then calls clearBuffer). */
int vrhip_set_fresnel(vrhip_ctx *ctx, float coef, float power);
/* replace cu_useCornellBox / cu_useExampleSphere / cu_useBRDF
 * (cuda/src/PathTracer.cu:976-989); flags travel by value in the launch. */
int vrhip_use_cornell_box(vrhip_ctx *ctx, int enable);
int vrhip_use_example_sphere(vrhip_ctx *ctx, int enable);
int vrhip_use_brdf(vrhip_ctx *ctx, int enable);
/* Traversal mode.  Default (0): children whose slab entry lies beyond the
 * closest hit so far (x 1.0009765625) are skipped -- the reference visits
 * every box the ray's line pierces (span end clamped to 1e20,
 * cuda/src/PathTracer.cu:316,322); skipping them leaves the closest hit
 * unchanged except in fp32 rounding corner cases.  1: visit
 * every pierced box exactly as the reference. */
int vrhip_set_strict_traversal(vrhip_ctx *ctx, int enable);

/* ---- scene uploads ---------------------------------------------------- */
/* replaces the device half of vRendererCuda::initMesh
 * (src/vRendererCuda.cpp:282-317) + cu_meshInitialised
 * (cuda/src/PathTracer.cu:997-1001): takes the flattened arrays in exactly
 * the reference layout (bvh: float4[n_bvh_f4], node = 4 float4 as in
 * :271-278; verts/normals/tangents: float4[n_slots]; uvs: float2[n_slots];
 * leaf runs end with a 0x80000000 terminator slot).  The library validates
 * the tree, records its depth and builds its own device layout. */
int vrhip_upload_mesh_flat(vrhip_ctx *ctx,
                           const float *bvh, size_t n_bvh_f4,
                           const float *verts, const float *normals,
                           const float *tangents, const float *uvs, size_t n_slots);
/* Convenience: indexed triangle mesh (vHVert/vHTriangle, include/vDataTypes.h)
 * -> native binned-SAH BVH -> reference flattening -> upload.  positions,
 * normals, tangents: float[3*n_verts]; uvs: float[2*n_verts] (may be NULL);
 * tris: uint32[3*n_tris]. */
int vrhip_upload_mesh_indexed(vrhip_ctx *ctx, const float *positions, const float *normals,
                              const float *tangents, const float *uvs, uint32_t n_verts,
                              const uint32_t *tris, uint32_t n_tris, uint32_t max_leaf_tris);
/* The same mesh from arrays that already live on the context's device (no
 * reference counterpart: the reference builds on the host, src/SBVH.cpp).
 * Every pointer is a device pointer; d_normals, d_tangents and d_uvs may be
 * NULL (zeros, as vrhip_build_flat); max_leaf_tris 0 means 2, at most 127.
 * The tree is built on the device: triangles in Morton order of their box
 * centres (ties by index), L = max(2, ceil(n_tris / max_leaf_tris)) leaves of
 * equal size (+-1), inner nodes halving the leaf range, depth ceil(log2 L); a
 * single triangle is stored twice under two leaves, as the host builder does.
 * The caller's data must be complete before the call or pending on the
 * context stream (see Streams at vrhip_set_stream); the build runs on the
 * context stream and the call returns when it has finished.  Transactional:
 * on any error the resident mesh stays as it was.  VRHIP_ERR_INVALID for null
 * or empty arrays, n_tris >= 2^24, max_leaf_tris > 127 (all before any device
 * call), an index >= n_verts or a non-finite position of a referenced vertex
 * (both found on the device), and on a vrhip_create_multi context (the
 * pointers live on one device).  Added without an ABI version change: ABI 6
 * gained this symbol, vrhip_export_mesh_flat and vrhip_selftest_half_box and
 * changed no other. */
int vrhip_upload_mesh_device(vrhip_ctx *ctx, const float *d_positions, const float *d_normals,
                             const float *d_tangents, const float *d_uvs, uint32_t n_verts,
                             const uint32_t *d_tris, uint32_t n_tris, uint32_t max_leaf_tris);
/* vrhip_upload_mesh_device with a choice of tree; everything said above holds
 * for both (arguments, checks and their order, transactional behaviour, the
 * refusal on a vrhip_create_multi context, "returns when the build has
 * finished"); an unknown builder is VRHIP_ERR_INVALID.
 *   VRHIP_DEVBVH_MORTON  the tree described above: exactly
 *     vrhip_upload_mesh_device, which forwards here.  Cheapest to build.
 *   VRHIP_DEVBVH_SAH  the tree vrhip_build_flat / vrhip_upload_mesh_indexed
 *     build on the host, built on the device: binned SAH with object splits,
 *     128 bins per axis over the centroid bounds, SAH costs 1 for a node and a
 *     triangle, the split after the first strictly cheapest bin (axes x, y, z
 *     in order), a leaf where max_leaf_tris allows one and splitting does not
 *     pay, coincident centroids halved by order, depth at most 30; a single
 *     triangle is stored twice under two leaves.  Every decision is taken from
 *     min/max boxes, counts and fp64 arithmetic, and the partition is stable,
 *     so vrhip_export_mesh_flat returns the node array of vrhip_build_flat
 *     byte for byte, with each leaf's triangles in ascending input index (the
 *     host's order inside a leaf may differ; boxes holding both -0 and +0 at an
 *     extreme may differ in that zero's sign).  vrhip_bvh_info reports the
 *     tree's real depth.  A leaf that would hold 128 or more triangles (only
 *     at the depth cap) is VRHIP_ERR_BVH, as it is for such a tree uploaded
 *     flat.  The host builder's experiment switches VRHIP_SAH_NODE_COST and
 *     VRHIP_SBVH_ALPHA are ignored.  Costs one small read-back per tree level.
 * Added without an ABI version change (ABI 6 gained this symbol and
 * vrhip_device_sah_scratch_bytes and changed no other). */
typedef enum vrhip_device_builder { VRHIP_DEVBVH_MORTON = 0, VRHIP_DEVBVH_SAH = 1 } vrhip_device_builder;
int vrhip_upload_mesh_device_ex(vrhip_ctx *ctx, const float *d_positions, const float *d_normals,
                                const float *d_tangents, const float *d_uvs, uint32_t n_verts,
                                const uint32_t *d_tris, uint32_t n_tris, uint32_t max_leaf_tris,
                                uint32_t builder);
/* Bytes of device scratch a VRHIP_DEVBVH_SAH build of n_tris triangles takes
 * while it runs (freed before the call returns); 0 without a device. */
size_t vrhip_device_sah_scratch_bytes(uint32_t n_tris);
/* New vertex positions for the resident mesh under an unchanged tree: a refit
 * (no reference counterpart), for a mesh that deforms from step to step.  The
 * resident mesh must have come from vrhip_upload_mesh_device or
 * vrhip_upload_mesh_device_ex, with either builder.  Topology stays exactly as
 * built: triangle indices, leaf membership, node numbering and order, the
 * triangles' root paths and the uvs.  All pointers are device pointers on the
 * context's device: d_positions float[3*n_verts], n_verts the upload's.
 * d_normals and d_tangents may each be NULL, and NULL here means KEEP what is
 * resident -- unlike the upload calls, where NULL means zeros.  After the
 * call the vertices (and the triangle test's precomputed edges, the same fp32
 * subtractions the build makes), and the normals / tangents where given, hold
 * the new data in the same slots; every child box is the exact fp32 min/max
 * box of the triangles beneath it, and every fp16 box its outward rounding, as
 * the builders write them.  Nodes are NOT re-sorted by area, so the kernels'
 * cached top of the tree may no longer hold the largest boxes: this changes
 * the rate only, never a result.  A refit tree degrades as the deformation
 * grows; vrhip_bvh_sah_cost is the number to decide on a rebuild with.
 * The work runs on the context stream and the call returns when it has
 * finished.  It does not clear the accumulation, as no upload does (call
 * vrhip_clear).  Transactional: a read-only pass first checks every referenced
 * position, and nothing resident is written unless it is clean.
 * VRHIP_ERR_INVALID (before any device call) for a null ctx or d_positions, no
 * resident mesh, a mesh from vrhip_upload_mesh_flat / _indexed (it keeps no
 * index data), n_verts different from the upload's, a vrhip_create_multi
 * context; and for a non-finite referenced position (found on the device).
 * Added without an ABI version change (ABI 6 gained this symbol,
 * vrhip_bvh_sah_cost and vrhip_flat_sah_cost and changed no other). */
int vrhip_refit_mesh_device(vrhip_ctx *ctx, const float *d_positions, const float *d_normals,
                            const float *d_tangents, uint32_t n_verts);
/* SAH cost of the resident tree, whichever call uploaded it, with the
 * builder's constants (1 per node, 1 per triangle):
 *   (sum over inner nodes of area(own box)
 *    + sum over leaves of area(leaf box) * triangle count) / area(root box),
 * area = dx*dy + dy*dz + dz*dx in fp64 from the fp32 boxes, a node's own box
 * the union of its two child boxes, the root included in the first sum.
 * Computed on the device in a fixed order (per-block partials, then one
 * block): two calls return the same bits.  Both this call and
 * vrhip_flat_sah_cost carry the sum as a pair of doubles with error-free
 * additions (error below 2^-100 of the sum), although the two visit the nodes
 * in different orders: in practice the device's value is the host's on the
 * exported tree bit for bit, and the tests assert that; it is no guarantee,
 * since a sum within 2^-100 of a rounding boundary of fp64 could still round
 * either way.  +infinity (and
 * VRHIP_OK) when the root's area is 0 or not finite.  VRHIP_ERR_INVALID with no mesh loaded.
 * Synchronous. */
int vrhip_bvh_sah_cost(vrhip_ctx *ctx, double *cost);
/* The resident mesh, whichever upload call brought it, rewritten on the host
 * in the reference layout vrhip_upload_mesh_flat takes (what the oracle, or a
 * caller caching a tree, needs of a device-built tree).  Nodes are numbered
 * by the LIFO flatten of vrhip_build_flat, so a tree that call made comes
 * back byte for byte; vertex .w is 0.  Call with NULL arrays for the sizes.
 * VRHIP_ERR_INVALID with no mesh loaded.  Synchronous. */
int vrhip_export_mesh_flat(vrhip_ctx *ctx, float *bvh, size_t *n_bvh_f4, float *verts, float *normals,
                           float *tangents, float *uvs, size_t *n_slots);
/* Ray queries against the resident mesh (no reference counterpart as a call:
 * the reference traces its own camera and bounce rays only): where does ray i,
 * origin d_origins[3i..], direction d_dirs[3i..], hit the mesh?  All pointers
 * are device pointers on the context's device; d_hits is 16-byte aligned.
 *   What is tested: the resident triangle mesh only.  The Cornell spheres, the
 *     small spheres and the example sphere are not part of the query, and the
 *     scene flags (vrhip_use_example_sphere included) have no effect on it.
 *   The test per triangle is the reference's intersectTriangle
 *     (cuda/include/RayIntersection.cuh:54-111) and closest-hit update
 *     (cuda/src/PathTracer.cu:379-386): fp32 without contraction, a hit needs
 *     dist > 3e-10 and dist < the closest so far (strict).  The closest so far
 *     starts at d_tmax[i], or at 1e20 (the reference's "no hit" distance) when
 *     d_tmax is NULL.  Directions are used as given, not normalised: t is in
 *     units of the direction's length.
 *   The record: t, the triangle, and the barycentrics u, v of that test.
 *     `prim` names the triangle in the caller's terms, by how the mesh came:
 *     vrhip_upload_mesh_device / _ex (also after any refit): the index of the
 *       triangle in the upload's d_tris;
 *     vrhip_upload_mesh_flat: the slot of the triangle's first vertex in the
 *       verts array as uploaded (the reference's own hit index);
 *     vrhip_upload_mesh_indexed: that slot in the arrays vrhip_build_flat
 *       returns for the same arguments;
 *     vrhip_flat_trace_rays: the slot in the arrays it was given.
 *   Ties: of two triangles hit at exactly the same t the one the reference's
 *     depth-first walk tests first wins, in both traversal modes
 *     (vrhip_set_strict_traversal selects the walk as for rendering; the
 *     results are identical).
 *   Miss: {t = d_tmax[i] (or 1e20), prim = VRHIP_RAY_MISS, u = 0, v = 0}.
 *   Every finite ray is answered, whatever its magnitudes, and as the
 *     reference's walk answers it: where its slab arithmetic overflows or
 *     cancels, that walk misses triangles a test of every triangle would
 *     accept, and so does this call.  The fp16 traversal mode is used only
 *     where it is known to return the reference walk's record: origin and
 *     mesh coordinates within 8 times the mesh's largest extent, no mesh
 *     coordinate beyond 65504, no non-zero direction component within 3e-10;
 *     every other ray is walked strictly in either mode.  Inside that range
 *     the equality of the two modes is what the tests pin, not a proof: a ray
 *     that grazes a node box within the last ulp may differ.  A finite ray
 *     whose arithmetic overflows may return a hit whose u or v is a NaN of
 *     unspecified sign and payload (the reference's `u < 0 || u > 1` lets a
 *     NaN through while dist stays finite).  t of a hit is never a NaN.
 *   Non-finite rays (one of the six floats not finite, or a NaN tmax) are
 *     classified before any traversal and reported as a miss with t = 1e20.
 *   VRHIP_RAYS_ANY (occlusion): only hit-or-miss is defined and the walk stops
 *     at the first accepted triangle: {0, 0, 0, 0} when some triangle is hit
 *     in (3e-10, tmax), the miss record otherwise; hit-or-miss equals the
 *     closest-hit query's for every ray.
 * The work runs on the context stream and the call returns when it has
 * finished.  It touches neither the accumulation, the images, the frame
 * counter nor the mesh.  n_rays == 0: VRHIP_OK, nothing written.
 * VRHIP_ERR_INVALID, before any device call, for a null ctx, null origins,
 * dirs or hits with n_rays > 0, misaligned hits, an unknown mode, no resident
 * mesh, and a vrhip_create_multi context (the pointers live on one device).
 * Added without an ABI version change (ABI 6 gained this symbol and
 * vrhip_flat_trace_rays and changed no other). */
#define VRHIP_RAY_MISS 0xffffffffu
typedef struct vrhip_ray_hit { float t; uint32_t prim; float u, v; } vrhip_ray_hit;   /* 16 B */
enum { VRHIP_RAYS_CLOSEST = 0, VRHIP_RAYS_ANY = 1 };
int vrhip_trace_rays(vrhip_ctx *ctx, const float *d_origins /*float[3n]*/, const float *d_dirs /*float[3n]*/,
                     const float *d_tmax /*float[n] or NULL*/, uint32_t n_rays, uint32_t mode,
                     vrhip_ray_hit *d_hits /*[n]*/);
/* Radiance queries (no reference counterpart as a call: the reference traces
 * its one camera only): what light arrives along the caller's own rays, for
 * irradiance probes, lightmap texels and radiance at arbitrary points.  The
 * reference's trace (cuda/src/PathTracer.cu:597-770) is run along n_rays rays
 * and one float4 per ray is written.  All arrays are device pointers on the
 * context's device; d_radiance is 16-byte aligned.
 *   Scene: the whole scene as vrhip_render would trace it right now -- Cornell
 *     box, example sphere, BRDF view, the resident mesh (ignored while the
 *     example sphere is on), texture maps, BRDF table, HDRI, Fresnel
 *     parameters -- under the flag word vrhip_render computes, walked as
 *     vrhip_set_strict_traversal says.  A mesh is not required.  The camera,
 *     the tiling, the frame counter, the accumulation and the images play no
 *     part and are not touched.
 *   Ray: the origin is used as given; the direction is normalised by the
 *     operation the reference applies to its camera ray (:842-844), so a
 *     caller who passes a pixel's un-normalised camera direction gets that
 *     pixel's camera ray.  A ray is valid when its six floats are finite and
 *     the fp32 sum dx*dx + dy*dy + dz*dz is finite and greater than 0.  An
 *     invalid ray is classified before any scene test; its record is
 *     {0, 0, 0, 0}.
 *   Paths: ray i starts from the seed pair (d_seeds[2i], d_seeds[2i+1]) and
 *     runs n_samples paths one after the other on that seed stream, exactly as
 *     the reference runs a pixel's two samples of a frame (:620-622): each
 *     path continues with the seeds the one before left behind.
 *     1 <= n_samples <= 4096.
 *   Record: rgb = ((0 + r_0 * c) + r_1 * c) + ... in path order, r_k path k's
 *     radiance and c = 1.f / (float)n_samples, every product and sum rounded
 *     in fp32: for n_samples = 2, bit for bit what the reference adds to a
 *     pixel in one frame (seeds (x * frame, y * time)).  w is the last path's
 *     result.w, the depth term: the depth image would show
 *     f2u8((1 - w) * 255).
 *   Range: rays are traced as the render traces its own.  Parity with the CPU
 *     oracle is pinned for origins at scene scale (tests/test_gpu_radiance.py);
 *     the extreme-float rules of vrhip_trace_rays (the strict walk for far
 *     origins, large coordinates and tiny direction components) are NOT
 *     applied here: a ray far outside the scene is walked like a camera ray
 *     placed there, and a record outside the tested range may hold NaNs.
 *   Cost: one ray per GPU lane; a lane whose paths end early idles until the
 *     slowest of its 64 neighbours has finished (no path pool for ray buffers).
 * The work runs on the context stream and the call returns when it has
 * finished.  n_rays == 0: VRHIP_OK, nothing written.  VRHIP_ERR_INVALID,
 * before any device call, for a null ctx, a null array with n_rays > 0, a
 * misaligned d_radiance, n_samples outside [1, 4096], and a
 * vrhip_create_multi context (the pointers live on one device).
 * VRHIP_ERR_NO_ENV in HDRI mode without an environment map, as vrhip_render.
 * Added without an ABI version change (ABI 6 gained this symbol and changed
 * no other). */
int vrhip_trace_radiance(vrhip_ctx *ctx, const float *d_origins /*float[3n]*/, const float *d_dirs /*float[3n]*/,
                         const uint32_t *d_seeds /*uint32[2n]*/, uint32_t n_rays, uint32_t n_samples,
                         float *d_radiance /*float4[n], 16-byte aligned*/);
/* Surface queries (no reference counterpart as a call): what does the path
 * tracer see at the first hit of the caller's own rays?  For denoiser guide
 * images (albedo, normal, depth), for the surface points and normals from
 * which probes and lightmap texels spawn their vrhip_trace_radiance rays, and
 * for picking.  The reference's intersectScene (cuda/src/PathTracer.cu:136-468)
 * is run once along each of n_rays rays and the vHitData record it leaves
 * (cuda/include/PathTracer.cuh:17-53), the one every bounce of trace computes
 * and consumes, is written out with what was hit.  All arrays are device
 * pointers on the context's device; d_hits is 16-byte aligned.
 *   Scene: the whole scene as vrhip_render would intersect it right now --
 *     Cornell box, the two small spheres, the example sphere, BRDF view, the
 *     resident mesh (ignored while the example sphere is on), texture maps --
 *     under the flag word vrhip_render computes, walked as
 *     vrhip_set_strict_traversal says.  A mesh is not required.  The camera,
 *     the tiling, the frame counter, the accumulation and the images play no
 *     part and are not touched.
 *   Ray: as vrhip_trace_radiance.  The origin is used as given; the direction
 *     is normalised by the operation the reference applies to its camera ray
 *     (:842-844), so t is in world units and a pixel's un-normalised camera
 *     direction (vrhip_camera_rays) gives that pixel's camera ray.  A ray is
 *     valid when its six floats are finite and the fp32 sum dx*dx + dy*dy +
 *     dz*dz is finite and greater than 0.  An invalid ray is classified before
 *     any scene test; its record is 28 zero words.
 *   Hit: position, normal, tangent, color, specular, emission and type are
 *     hitPoint, normal, tangent, color, spec, emission (xyz) and hitType of the
 *     closest hit, the values bounce 0 of trace sees, quirks included: the
 *     normal is the normal-mapped one where a normal map is loaded (and the
 *     tangent is usable), the face normal otherwise; color is the base colour
 *     after the diffuse map; the example sphere's texture coordinates come from
 *     the normal the previous hit of the same call left behind (:202-204).
 *     type: 0 specular, 1 diffuse, 2 BRDF.
 *     kind and prim say what was hit: VRHIP_SURF_CORNELL with prim 0-5 (the
 *     light, then the walls, in the reference's order, :113-121),
 *     VRHIP_SURF_SMALL with prim 0-1 (:107-111), VRHIP_SURF_EXAMPLE with prim
 *     0, VRHIP_SURF_MESH with the triangle in the caller's terms exactly as
 *     vrhip_trace_rays defines prim, also after a refit.
 *     bary_u, bary_v: the triangle test's barycentrics for a mesh hit, 0
 *     otherwise.  tex_u, tex_v: the interpolated texture coordinates of a
 *     mesh hit, (b0 * uv0 + u * uv1) + v * uv2 with b0 = 1 - u - v in fp32, 0
 *     otherwise.  pad0 and pad1 are 0.
 *   Miss: t = 1e20, kind = VRHIP_SURF_NONE, prim = VRHIP_RAY_MISS, every other
 *     word 0.
 *   Range: as vrhip_trace_radiance.  Parity with the CPU oracle is pinned for
 *     origins at scene scale (tests/test_gpu_surface.py); the extreme-float
 *     rules of vrhip_trace_rays are NOT applied here, and a record outside the
 *     tested range may hold NaNs.  In the tested range a mesh hit's t, prim
 *     and barycentrics are vrhip_trace_rays's for the normalised direction.
 *   Cost: one ray per GPU lane, seven 16-byte stores per ray.
 * The work runs on the context stream and the call returns when it has
 * finished.  It touches nothing resident.  n_rays == 0: VRHIP_OK, nothing
 * written.  VRHIP_ERR_INVALID, before any device call, for a null ctx, a null
 * array with n_rays > 0, a misaligned d_hits, and a vrhip_create_multi context
 * (the pointers live on one device).  VRHIP_ERR_NO_ENV in HDRI mode without an
 * environment map, exactly where vrhip_trace_radiance returns it.
 * Added without an ABI version change (ABI 6 gained this symbol and
 * vrhip_camera_rays and changed no other). */
enum { VRHIP_SURF_NONE = 0, VRHIP_SURF_CORNELL = 1, VRHIP_SURF_SMALL = 2,
       VRHIP_SURF_EXAMPLE = 3, VRHIP_SURF_MESH = 4 };
typedef struct vrhip_surface_hit {       /* 112 B = 7 float4, 16-byte aligned */
    float t; uint32_t kind, prim, type;  /* type: vHitData hitType, 0 specular 1 diffuse 2 BRDF */
    float position[3], bary_u;
    float normal[3],   bary_v;
    float tangent[3],  pad0;             /* 0 */
    float color[3],    tex_u;
    float specular[3], tex_v;
    float emission[3], pad1;             /* 0 */
} vrhip_surface_hit;
int vrhip_trace_surface(vrhip_ctx *ctx, const float *d_origins /*float[3n]*/, const float *d_dirs /*float[3n]*/,
                        uint32_t n_rays, vrhip_surface_hit *d_hits /*[n], 16-byte aligned*/);
/* The current camera's rays as a buffer: for every pixel of the W x H image,
 * row-major (pixel (x, y) at y * W + x, every pixel whatever the tiling), the
 * camera origin and the UN-normalised direction (dir + cx * sx) + cy * sy of
 * the reference's camera ray (cuda/src/PathTracer.cu:833-844, no jitter), the
 * operand of its normalize, from the table and in the operation order the
 * render kernels use.  vrhip_trace_surface and vrhip_trace_radiance normalise
 * it as those kernels do and so trace the pixel's camera ray bit for bit;
 * vrhip_trace_rays takes directions as given (its t is then in units of this
 * direction's length).  Device pointers on the context's device, float[3 W H]
 * each.  Runs on the context stream and returns when it has finished; closes
 * a render-service session; touches nothing resident.  VRHIP_ERR_INVALID,
 * before any device call, for a null ctx, a null array, and a
 * vrhip_create_multi context. */
int vrhip_camera_rays(vrhip_ctx *ctx, float *d_origins /*float[3*W*H]*/, float *d_dirs /*float[3*W*H]*/);
/* The surface record at a point of the resident mesh, with no ray (no
 * reference counterpart): the record vrhip_trace_surface would write for a hit
 * of triangle prims[i] at barycentrics (u, v) = d_bary[2i], d_bary[2i + 1].
 *   prim: the triangle exactly as vrhip_trace_rays names it: after
 *     vrhip_upload_mesh_device[_ex] (also after a refit) the row of tris, after
 *     vrhip_upload_mesh_flat / _indexed the flat slot of its first vertex.
 *   u, v are used as given, not clamped: extrapolation is the caller's business.
 *   Record: kind = VRHIP_SURF_MESH, prim, bary_u = u, bary_v = v, t = 0.
 *     position has no hit-point form without a ray: per component it is
 *     (b0 * v0 + u * v1) + v * v2 in fp32 with b0 = 1.f - u - v evaluated left
 *     to right, the shape of tex_u and tex_v.  Every other word is what the
 *     mesh hit of vrhip_trace_surface holds, computed by the same device code on
 *     the same operands in the same order: the mapped normal where a normal map
 *     is loaded and the tangent is usable and the face normal otherwise, the
 *     tangent, color after the diffuse map, specular, emission 0, type 2 under
 *     the BRDF view and 1 otherwise, tex_u, tex_v; the pads are 0.
 *   Scene: the maps and the BRDF-view flag apply as vrhip_render would apply
 *     them now; the Cornell-box and example-sphere flags have no effect, as in
 *     vrhip_trace_rays; no environment map is needed.
 *   Invalid: an entry whose prim names no resident triangle (out of range, a
 *     flat slot that is no triangle's first vertex, VRHIP_RAY_MISS) or whose u
 *     or v is not finite gives 28 zero words; it is classified before any
 *     attribute load.
 * The prim -> triangle lookup is the inverse of what vrhip_trace_rays reports;
 * it is built on the device at the first call after an upload (where a caller
 * triangle is stored more than once, the first stored copy is taken) and kept
 * until the next upload; a refit keeps it.  Nothing else resident is touched.
 * Runs on the context stream and returns when it has finished; closes a
 * render-service session.  VRHIP_ERR_INVALID, before any device call, for a
 * null ctx, a null array with n > 0, a misaligned d_hits, a
 * vrhip_create_multi context, and no mesh loaded, checked in that order and
 * whatever n is: as in vrhip_trace_rays the mesh comes before "nothing to do".
 * Then n == 0: VRHIP_OK, nothing written, no device call.
 * Added without an ABI version change. */
int vrhip_surface_at(vrhip_ctx *ctx, const uint32_t *d_prims /*[n]*/, const float *d_bary /*float[2n]: u, v*/,
                     uint32_t n, vrhip_surface_hit *d_hits /*[n], 16-byte aligned*/);
/* The surface records of a width x height lightmap atlas of the resident
 * mesh's uvs (no reference counterpart): the first stage of a bake,
 *   vrhip_atlas_surface -> vrhip_shade_surface -> vrhip_denoise ->
 *   vrhip_upload_texture(diffuse) -> vrhip_render.
 * Texel (x, y) is record y * width + x; its centre is
 *   cx = ((double)x + 0.5) / (double)width, cy = ((double)y + 0.5) / (double)height,
 * so the texel the renderer's map fetch addresses for (u, v) -- x = (int)(width
 * * u), y = (int)(height * v) -- is the texel that contains (u, v).
 * THE DEFINITION.  Everything is fp64 + - * / without contraction, correctly
 * rounded; no sqrt, no libm.
 *   Triangle: the uvs a, b, c of its three vertex slots widened to double.  A
 *     triangle with a non-finite uv covers nothing.
 *   Edge function, canonical per edge: order the endpoints of edge (p, q) as
 *     p' < q' by (x, then y);
 *       E = (q'x - p'x) * (cy - p'y) - (q'y - p'y) * (cx - p'x),
 *     negated if the endpoints were swapped.  Two triangles that share an edge
 *     compute the same magnitude with opposite signs, so a texel centre on a
 *     shared edge is never lost between them.
 *   Coverage: A2 is the edge function of (a, b) evaluated at c.  A2 == 0 or
 *     not finite: the triangle covers nothing.  A2 > 0: the centre is covered
 *     iff the edge values of (a, b), (b, c), (c, a) are all >= 0; A2 < 0: iff
 *     all three are <= 0.  Both windings count (mirrored charts are legal).
 *   Winner: among the triangles that cover a centre the smallest prim (in the
 *     caller's terms, as vrhip_surface_at) wins, whatever the builder, the tree
 *     and the order the triangles are stored in.
 *   Barycentrics of the winner, plain (not canonical) forms, c.x, c.y vertex c:
 *       eu = (cx - a.x) * (c.y - a.y) - (cy - a.y) * (c.x - a.x),
 *       ev = (b.x - a.x) * (cy - a.y) - (b.y - a.y) * (cx - a.x),
 *       ud = eu / A2, vd = ev / A2,
 *       u = (float)clamp(ud, 0, 1), v = (float)clamp(vd, 0, 1)
 *     (clamp(x, 0, 1) = x < 0 ? 0 : x > 1 ? 1 : x), and if the fp32 sum
 *     u + v > 1.f then v = 1.f - u.
 *   Record: a covered texel gets vrhip_surface_at(prim, u, v)'s record, t = 0;
 *     an uncovered one the miss record of vrhip_trace_surface (t = 1e20, kind
 *     0, prim VRHIP_RAY_MISS, every other word 0).
 *   Gutter: `gutter` dilation passes, 0 to 64.  In pass k = 1 .. gutter a texel
 *     still uncovered after pass k - 1 looks at its eight neighbours in the
 *     order (x-1,y) (x+1,y) (x,y-1) (x,y+1) (x-1,y-1) (x+1,y-1) (x-1,y+1)
 *     (x+1,y+1), those inside the atlas only (no wrap), and takes the (prim, u,
 *     v) of the first that was covered after pass k - 1; its record is that
 *     neighbour's with t = (float)k.  vrhip_shade_surface and vrhip_denoise do
 *     not read t; here it is the texel's distance from coverage.  The gutter
 *     exists because the renderer fetches maps by truncation: a hit near a
 *     chart's border can land in a texel whose centre the chart does not
 *     cover, and without a gutter that texel of the baked map is black.
 *   Limits: 1 <= width, height <= 16384, width * height <= 2^26.
 * Scene dependence as vrhip_surface_at.  Runs on the context stream and
 * returns when it has finished; closes a render-service session; touches
 * nothing resident.  VRHIP_ERR_INVALID, before any device call, for a null
 * ctx, a null or misaligned d_hits, a size or gutter out of range, a
 * vrhip_create_multi context, and no mesh loaded.
 * Cost: scratch of 32 bytes per texel kept with the context; one 64-bit integer
 * atomic minimum per (covering triangle, texel), seven 16-byte stores per
 * texel (profiles/atlas).  Added without an ABI version change. */
int vrhip_atlas_surface(vrhip_ctx *ctx, uint32_t width, uint32_t height, uint32_t gutter,
                        vrhip_surface_hit *d_hits /*[width*height], 16-byte aligned*/);
/* Radiance from the caller's surface records (no reference counterpart as a
 * call): what would the renderer show for this surface, seen from this
 * direction?  For lightmap texels and irradiance probes, whose points and
 * normals come from a UV unwrap or a probe grid and were never reached by a
 * ray, and for relighting the records of vrhip_trace_surface with other
 * materials.  The reference's trace (cuda/src/PathTracer.cu:597-770) is run
 * with the result of bounce 0's intersectScene given by the caller: a miss
 * takes :631-652 along the direction, a hit takes :664-764 with the record as
 * vHitData; bounces 1 to 3 are the render's own.  One float4 per record is
 * written.  All arrays are device pointers on the context's device; d_hits and
 * d_radiance are 16-byte aligned.
 *   Scene: as vrhip_trace_radiance -- the whole scene as vrhip_render would
 *     trace it right now, under its flag word, walked as
 *     vrhip_set_strict_traversal says.  A mesh is not required.
 *   Record: kind is read only as 0 = miss, 1..4 = hit.  Of a hit position,
 *     normal, tangent, color, specular, emission (xyz, w taken as 0) and type
 *     are read; t, prim, the barycentrics, tex_u, tex_v and the pads are not.
 *     The normal is used as given and is NOT normalised (the reference uses a
 *     unit hit.normal; pass one).  Non-finite values and zero vectors in a
 *     record propagate as the render's arithmetic propagates them: a zero
 *     normal gives NaN radiance.  d_dirs[3i..3i+2] is the incoming direction
 *     of record i (the ray that arrives at the surface, pointing at it),
 *     normalised by the operation the other queries use.  A record is invalid
 *     when a float of its direction is not finite or the fp32 sum dx*dx +
 *     dy*dy + dz*dz is not finite and greater than 0, when kind > 4, or when it
 *     is a hit with type > 2.  An invalid record is classified before any scene
 *     work; its result is {0, 0, 0, 0}.
 *   Paths: as vrhip_trace_radiance -- record i runs n_samples paths one after
 *     the other on the seed stream (d_seeds[2i], d_seeds[2i+1]).
 *     1 <= n_samples <= 4096.
 *   Result: rgb = ((0 + r_0 * c) + r_1 * c) + ... in path order with
 *     c = 1.f / (float)n_samples, every product and sum rounded in fp32.
 *     w = 0: without a camera origin there is no depth term.
 *   Consequences:
 *     1. vrhip_trace_surface(o, d) followed by this call with the same d,
 *        seeds and n_samples gives the rgb of vrhip_trace_radiance(o, d, ...)
 *        bit for bit, in both traversal modes.
 *     2. A record with type = 1, specular.x = 0 and emission = 0 does not
 *        depend on its direction (the Fresnel draw is still taken and
 *        discarded, :678-722).  With color = (1, 1, 1) it is what a lightmap
 *        texel or an irradiance probe stores: the reference's diffuse estimate
 *        at that point and normal.  It is not an irradiance in W/m^2: it
 *        carries the reference's own weight 2 * cos on a cosine-distributed
 *        sample (for a uniform incoming radiance L it converges to
 *        2 * E[cos] * L = 4/3 L, where L is the physical answer).  The factor
 *        is the reference's and is not corrected.
 *     3. Range: as vrhip_trace_radiance.  Parity with the CPU oracle is pinned
 *        for points at scene scale (tests/test_gpu_shade.py); there is no
 *        extreme-float walk.
 *   Cost: one record per GPU lane, as vrhip_trace_radiance: a lane whose paths
 *     end early idles until the slowest of its 64 neighbours has finished.
 *     (Lanes that take the next record at once were built and measured and
 *     did not win on the Cornell box)
 * The work runs on the context stream and the call returns when it has
 * finished.  It closes a render-service session and touches nothing resident.
 * n_hits == 0: VRHIP_OK, nothing written.  VRHIP_ERR_INVALID, before any device
 * call, for a null ctx, a null array with n_hits > 0, a misaligned d_hits or
 * d_radiance, n_samples outside [1, 4096], and a vrhip_create_multi context.
 * VRHIP_ERR_NO_ENV in HDRI mode without an environment map, exactly where
 * vrhip_trace_radiance returns it.  Added without an ABI version change (ABI 6
 * gained this symbol and changed no other). */
int vrhip_shade_surface(vrhip_ctx *ctx, const vrhip_surface_hit *d_hits /*[n], 16-byte aligned*/,
                        const float *d_dirs /*float[3n]*/, const uint32_t *d_seeds /*uint32[2n]*/,
                        uint32_t n_hits, uint32_t n_samples, float *d_radiance /*float4[n], 16-byte aligned*/);
/* Probe query (no reference counterpart as a call): radiance from n_probes
 * points along one shared set of n_dirs directions, projected onto real
 * spherical harmonics (SH) to band 2 inside the call, and the call that turns
 * the coefficients back into irradiance at a normal.  The loop of an irradiance
 * probe grid: vrhip_probe_sh -> vrhip_sh_irradiance.  No buffer of
 * n_probes * n_dirs elements is allocated; the call's scratch is at most
 * n_probes * ceil(n_dirs / 64) * 112 bytes.  All arrays are device pointers on
 * the context's device; d_sh is 16-byte aligned.
 *   Ray (i, k): exactly the ray vrhip_trace_radiance would trace with origin
 *     d_points[3i..], direction d_dirs[3k..], the seed pair
 *     (d_probe_seeds[2i] ^ d_dir_seeds[2k],
 *      d_probe_seeds[2i+1] ^ d_dir_seeds[2k+1]) and n_samples paths, one after
 *     the other.  Its validity rule, normalisation, shared escape under an
 *     HDRI and path-order mean are that query's own, and so are the scene, the
 *     flag word, the traversal mode, the session handling and the order of
 *     refusals.  L = the rgb of the record that call would return, d =
 *     (x, y, z) the normalised direction it traced.  A ray is invalid when the
 *     point is not finite or the direction fails that query's rule.
 *   Basis: in fp32, every product and sum rounded on its own, in this order:
 *       Y0 = 0.282094792f
 *       Y1 = 0.488602512f*y    Y2 = 0.488602512f*z    Y3 = 0.488602512f*x
 *       Y4 = 1.09254843f*(x*y) Y5 = 1.09254843f*(y*z)
 *       Y6 = 0.315391565f*(3.f*(z*z) - 1.f)
 *       Y7 = 1.09254843f*(x*z) Y8 = 0.546274215f*(x*x - y*y)
 *   Term: t[j][c] = (w_k * Y_j) * L[c], w_k = d_weights[k] used as given (NaN
 *     and inf propagate), or 12.566370614f / (float)n_dirs with d_weights
 *     NULL.  An invalid ray's term is +0.f whatever its weight (not w*Y*0).
 *   Sum: directions are taken in blocks of VRHIP_PROBE_BLOCK = 64 consecutive
 *     k.  Slot l of block b holds the term of direction 64b + l, or +0.f
 *     beyond n_dirs.  The 64 slots are added by the fixed tree
 *       for s in 32, 16, 8, 4, 2, 1: for l < s: v[l] = v[l] + v[l + s]
 *     and the block partials v[0] are added in ascending b, starting from
 *     +0.f.  The order does not depend on the grid, on residency or on how the
 *     work is split over launches; there are no floating-point atomics.
 *   Record: VRHIP_PROBE_WORDS = 28 words per probe.  Word 3j + c is coefficient
 *     j of channel c; word 27 is a uint32, the number of valid rays of the
 *     probe.
 *   Range: as vrhip_trace_radiance.  Parity with the CPU oracle is pinned for
 *     points at scene scale (tests/test_gpu_probe.py).
 *   Cost: one wave per (probe, block), lane l tracing direction 64b + l; the
 *     lanes of a block share a wave, so directions that are close together in
 *     a block walk the scene together.
 * 1 <= n_samples <= 4096, 1 <= n_dirs <= 65536.  The work runs on the context
 * stream and the call returns when it has finished.  It closes a render-service
 * session and touches nothing resident.  n_probes == 0: VRHIP_OK, nothing
 * written.  VRHIP_ERR_INVALID, before any device call, for a null ctx, a null
 * array other than d_weights with n_probes > 0, a misaligned d_sh, n_samples or
 * n_dirs out of range, and a vrhip_create_multi context.  VRHIP_ERR_NO_ENV in
 * HDRI mode without an environment map, exactly where vrhip_trace_radiance
 * returns it.  VRHIP_ERR_NOMEM when the scratch cannot be allocated.  Added
 * without an ABI version change (ABI 6 gained this symbol and changed no
 * other). */
#define VRHIP_PROBE_BLOCK 64
#define VRHIP_PROBE_WORDS 28
int vrhip_probe_sh(vrhip_ctx *ctx, const float *d_points /*float[3 n_probes]*/,
                   const float *d_dirs /*float[3 n_dirs], shared by all probes*/,
                   const float *d_weights /*float[n_dirs] or NULL*/,
                   const uint32_t *d_probe_seeds /*uint32[2 n_probes]*/, const uint32_t *d_dir_seeds /*uint32[2 n_dirs]*/,
                   uint32_t n_probes, uint32_t n_dirs, uint32_t n_samples,
                   float *d_sh /*float4[7 n_probes] = 28 words per probe, 16-byte aligned*/);
/* Irradiance at a normal from the records of vrhip_probe_sh; needs no scene and
 * no mesh.  Output q takes record p = d_index ? d_index[q] : q of the m records
 * and the normal (x, y, z) = d_normals[3q..], used as given (not normalised, as
 * vrhip_shade_surface treats normals).  With Y0..Y8 the basis above on the
 * normal, A0 = 3.14159274f, A1 = 2.09439516f, A2 = 0.785398185f (the
 * clamped-cosine lobe of Ramamoorthi and Hanrahan, "An Efficient Representation
 * for Irradiance Environment Maps", SIGGRAPH 2001) and A(j) = A0 for j = 0, A1
 * for j = 1..3, A2 for j = 4..8, per channel c in fp32, every product and sum
 * rounded on its own, left to right in j:
 *   E[c] = ((A(0)*(sh[0][c]*Y0) + A(1)*(sh[1][c]*Y1)) + ...) + A(8)*(sh[8][c]*Y8)
 * out = (E.r, E.g, E.b, 0); d_index[q] >= m gives (0, 0, 0, 0).  n == 0:
 * VRHIP_OK, nothing written.  VRHIP_ERR_INVALID, before any device call, for a
 * null ctx, a null d_sh, d_normals or d_out with n > 0, a misaligned d_out,
 * d_index NULL with n > 0 and n != m, and a vrhip_create_multi context.  Synchronous;
 * closes a render-service session.  Added without an ABI version change. */
int vrhip_sh_irradiance(vrhip_ctx *ctx, const float *d_sh /*28 words per probe, m probes*/, uint32_t m,
                        const uint32_t *d_index /*uint32[n] or NULL (then n == m, identity)*/,
                        const float *d_normals /*float[3n]*/, uint32_t n, float *d_out /*float4[n], 16-byte aligned*/);
/* Edge-avoiding a-trous denoiser (no reference counterpart: the reference shows
 * its accumulation unfiltered; Dammertz et al., "Edge-Avoiding A-Trous Wavelet
 * Transform for fast Global Illumination Filtering", HPG 2010).  The step
 * between the guides vrhip_trace_surface produces and an image: for a view at
 * a few paths per pixel, a lightmap atlas, a probe sheet.  vrhip_denoise
 * filters caller buffers of any grid and needs no scene and no mesh;
 * vrhip_denoise_frame filters the context's own accumulation.
 *   Grid: width x height cells, row-major (cell (x, y) at y * width + x).
 *     color: float4 per cell, the mean radiance in rgb; w is carried through
 *     untouched.  guides: one vrhip_surface_hit per cell; read are kind,
 *     position P, normal N (used as given) and color, the albedo A.
 *   Valid: a cell with 1 <= kind <= 4.  A miss, an invalid record and
 *     kind > 4 make a cell invalid: it keeps its colour through every pass and
 *     contributes to no other cell.
 *   Arithmetic: fp32, no contraction, in exactly the order written here;
 *     1.f / x is the IEEE quotient.  kp = 1.f / (sigma_position *
 *     sigma_position); kc_0 = 1.f / (sigma_color * sigma_color); kc_j = kc_0 *
 *     (float)(1u << 2j), which halves the colour sigma each pass; K = {0.375f,
 *     0.25f, 0.0625f}, the B3 spline.
 *   Demodulation (VRHIP_DENOISE_DEMODULATE, n_passes > 0): for a valid cell
 *     and a channel with A.ch > 0x1p-8f, C.ch = color.ch * (1.f / A.ch) is
 *     filtered and out.ch = C.ch * A.ch after the last pass; other channels and
 *     other cells are filtered as given.
 *   Pass j = 0 .. n_passes - 1, s = 1 << j, for a valid cell p = (x, y):
 *       sum = 0 (three channels), ws = 0
 *       for dy in -2..2 (outer), dx in -2..2 (inner):
 *           q = (x + dx*s, y + dy*s); skipped when outside the grid or invalid
 *                                     (no clamping, no mirroring)
 *           h  = K[|dy|] * K[|dx|]
 *           dn = (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z
 *           wn = dn > 0 ? dn : 0   (a NaN gives 0); m times: wn = wn * wn
 *           e  = P_q - P_p
 *           dp = (N_p.x*e.x + N_p.y*e.y) + N_p.z*e.z
 *           wp = 1.f / (1.f + (dp*dp) * kp)
 *           dc = C_q - C_p
 *           d2 = (dc.x*dc.x + dc.y*dc.y) + dc.z*dc.z
 *           wc = 1.f / (1.f + d2 * kc_j)
 *           w  = ((h * wn) * wp) * wc
 *           sum.ch = sum.ch + w * C_q.ch;  ws = ws + w
 *     with m = normal_power_log2.  When ws > 0 the new colour is C'.ch =
 *     sum.ch * (1.f / ws), otherwise C' = C_p.  The weights are rational on
 *     purpose: no transcendental function, so a plain C restatement
 *     (tests/denoise_driver.c) gives the kernels' bits.  NaNs and infinities in
 *     colours or guides propagate as this arithmetic propagates them.
 *     n_passes = 0 copies color to out bit for bit.
 *   Params: n_passes 0 to 8, normal_power_log2 0 to 8, flags 0 or
 *     VRHIP_DENOISE_DEMODULATE, both sigmas finite and greater than 0.
 *   Cost: memory-bound; per pass three float4 planes read and one written per
 *     cell, from four float4 planes of scratch the context keeps (64 bytes a
 *     cell, grown on demand, freed by vrhip_destroy).
 * vrhip_denoise: device pointers on the context's device, 16-byte aligned;
 * d_out may equal d_color.  Runs on the context stream and returns when it has
 * finished; closes a render-service session; touches nothing resident.
 * VRHIP_ERR_INVALID, before any device call, for a null ctx, a null array, a
 * misaligned array, a width or height of 0 or width * height >= 2^31, null
 * params, n_passes > 8, normal_power_log2 > 8, unknown flags, a sigma that is
 * not finite and greater than 0, and a vrhip_create_multi context.
 * VRHIP_ERR_NOMEM when the scratch cannot be allocated; nothing has changed.
 * vrhip_denoise_frame: color = accum * (1.f / (float)frames) by the tonemap's
 * own operation (rgb scaled, w as accumulated); guides = vrhip_trace_surface
 * on vrhip_camera_rays, made in library scratch (136 more bytes a pixel; not
 * made when n_passes = 0).  Writes d_out_f32 (float4[W*H], 16-byte aligned)
 * and / or d_out_rgba8 (uchar4[W*H]: tone_byte(clampf(c, 0, 1)) per channel
 * with the render's own threshold table, alpha 0xff; with n_passes = 0 the
 * bytes of vrhip_read_rgba8); either may be NULL, not both.  The accumulation,
 * the context's own images and the frame counter are not touched.
 * VRHIP_ERR_INVALID, before any device call, for a null ctx, two null
 * outputs, a misaligned output, the parameter errors above, a
 * vrhip_create_multi context, a tiled rank (n_ranks > 1: its accumulation
 * holds only its own tiles), 2^31 pixels or more, and when no frame has been
 * rendered since the last clear.  VRHIP_ERR_NO_ENV in HDRI mode without an
 * environment map, as vrhip_trace_surface.
 * Added without an ABI version change (ABI 6 gained these symbols and changed
 * no other). */
enum { VRHIP_DENOISE_DEMODULATE = 1 };
typedef struct vrhip_denoise_params {
    uint32_t n_passes, flags, normal_power_log2;
    float sigma_color, sigma_position;
} vrhip_denoise_params;
int vrhip_denoise(vrhip_ctx *ctx, const float *d_color /*float4[w*h]*/, const vrhip_surface_hit *d_guides /*[w*h]*/,
                  uint32_t width, uint32_t height, const vrhip_denoise_params *params, float *d_out /*float4[w*h]*/);
int vrhip_denoise_frame(vrhip_ctx *ctx, const vrhip_denoise_params *params, float *d_out_f32 /*float4[W*H] or NULL*/,
                        uint8_t *d_out_rgba8 /*uchar4[W*H] or NULL*/);
/* replaces vRendererCuda::loadHDR (src/vRendererCuda.cpp:320-340) +
 * cu_setHDRDim: rgba float4[w*h] (or half4 with the _half variant, the
 * Imf::Rgba layout, converted on the device). */
int vrhip_upload_hdr(vrhip_ctx *ctx, const float *rgba, uint32_t w, uint32_t h);
int vrhip_upload_hdr_half(vrhip_ctx *ctx, const uint16_t *rgba_half, uint32_t w, uint32_t h);
/* replaces the device half of vRendererCuda::loadTexture
 * (src/vRendererCuda.cpp:342-411) + cu_bindTexture: rgba float4[w*h]
 * (already gamma-converted by the caller, as the reference host does). */
int vrhip_upload_texture(vrhip_ctx *ctx, int type, const float *rgba, uint32_t w, uint32_t h);
/* replaces the device half of vRendererCuda::loadBRDF
 * (src/vRendererCuda.cpp:413-437) + cu_bindBRDF: float[3*90*90*180] planar
 * R,G,B MERL table.  Copies (interleaving the channels on the device, so a
 * lookup reads one cache line); does NOT take ownership (the C++ adapter
 * reproduces the reference's delete[]). */
int vrhip_upload_brdf(vrhip_ctx *ctx, const float *table, size_t n_floats);

/* replaces vBRDFLoader::loadBinary (src/BRDFLoader.cpp:15-50): reads a MERL
 * .binary file (3 int32 dims, then 3*90*90*180 doubles, planar R,G,B) into
 * `table` as floats in the same order.  Host only; the caller passes the
 * table to vrhip_upload_brdf.  VRHIP_ERR_INVALID on a dimension mismatch or
 * short file (the reference prints and returns nullptr). */
int vrhip_load_merl(const char *path, float *table, size_t n_floats);

/* replaces the OpenEXR read in NGLScene::loadHDRMap (src/NGLScene.cpp:205-231,
 * Imf::RgbaInputFile over the data window): a single-part scanline .exr
 * (NONE, RLE, ZIPS or ZIP compression; HALF/FLOAT/UINT channels) as half RGBA
 * (Imf::Rgba layout, FLOAT samples rounded to half; missing R/G/B = 0,
 * A = 1), ready for vrhip_upload_hdr_half.  Pass rgba_half = NULL to query
 * the size.  Host only. */
int vrhip_load_exr(const char *path, uint16_t *rgba_half, size_t n_values, uint32_t *width, uint32_t *height);

/* ---- display interop ---------------------------------------------------- */
/* replaces vRendererCuda::registerTextureBuffer / registerDepthBuffer
 * (src/vRendererCuda.cpp:57-67): registers an OpenGL texture (which = 0:
 * colour, 1: depth; target e.g. GL_TEXTURE_2D = 0x0DE1) with HIP.  Needs the
 * caller's GL context current. */
int vrhip_gl_register_image(vrhip_ctx *ctx, int which, unsigned int gl_texture, unsigned int gl_target);
/* Copies the RGBA8 colour and depth images into the registered textures
 * (map, device-to-array copy, unmap); the reference's kernel wrote them
 * through surfaces (src/vRendererCuda.cpp:117-162). Synchronous. */
int vrhip_gl_present(vrhip_ctx *ctx);

/* ---- rendering -------------------------------------------------------- */
/* replaces vRendererCuda::render (src/vRendererCuda.cpp:107-165) +
 * cu_runRenderKernel (cuda/src/PathTracer.cu:870-892), for n_frames
 * consecutive frames in one device pass.  times[i] is the _time RNG seed of
 * frame i (the reference uses wall-clock ms); times may be NULL, then
 * `time_seed` is used for every frame.  Enqueues and returns; call
 * vrhip_sync for the reference's synchronous behaviour.  The path kernels
 * run on the context stream or, behind a launch still in flight, on the
 * context's three internal path streams (see vrhip_set_overlap);
 * the finish pass that writes the accumulation, colour and depth images runs
 * on the context stream after them, so work queued on the context stream
 * afterwards (reads, vrhip_pack_tiles, a collective) sees the results. */
int vrhip_render(vrhip_ctx *ctx, uint32_t n_frames, const uint32_t *times, uint32_t time_seed);
/* Same render, through the counting kernel variant (identical results, plus
 * per-event counts for the roofline's algorithmic bytes):
 * counters[0..7] = rays (intersectScene calls), inner-node visits (64 B),
 * terminator slot reads (16 B; 0 with the device layout), triangle tests
 * (48 B), hit
 * attribute bytes, texture fetches (16 B), HDRI fetches (16 B), BRDF lookups
 * (12 B).  Synchronous. */
int vrhip_render_counted(vrhip_ctx *ctx, uint32_t n_frames, const uint32_t *times, uint32_t time_seed,
                         uint64_t counters[8]);
/* Same render as vrhip_render -- the production kernels' algorithm (t-culled
 * traversal unless strict, primary hit shared by a pixel's paths, last bounce
 * without material sampling), the scene specialisation's launch shape
 * (block size, waves per SIMD, node-loop threshold, work queues) and results
 * -- through an instrumented instantiation of that specialisation that
 * counts the memory operations its kernels issue (the roofline's executed
 * bytes; no reference counterpart).  Launches of one frame take the primary
 * pass here (production traces their camera rays in the path kernel), and
 * counting launches never overlap a launch in flight.
 * counters[0..7] as vrhip_render_counted but for the executed work
 * (attribute bytes include the 36 B of vertices a mesh hit's face normal
 * reads), then [8] node visits served from the block's LDS copy of the tree
 * top, [9] triangle loads issued
 * (36 B each; an odd leaf's last pair loads its triangle twice), [10] mesh
 * hits shaded, [11] of those through the normal map, [12..15] every global
 * lane load the production kernels issue, by width: 16 B, 12 B, 8 B, 4 B
 * (nodes, triangles, primary records, attributes, texels, BRDF entries),
 * [16] paths that took their pixel's shared escape radiance (sphere-only HDRI
 * scenes: a camera ray that escapes gives every path of the pixel the same
 * result, fetched once per pixel and launch).
 * Synchronous. */
#define VRHIP_PROFILE_COUNTERS 17
int vrhip_render_profiled(vrhip_ctx *ctx, uint32_t n_frames, const uint32_t *times, uint32_t time_seed,
                          uint64_t counters[VRHIP_PROFILE_COUNTERS]);
/* Waits until every render queued on the context is complete: the
 * accumulation, colour and depth images hold it (cudaStreamSynchronize in
 * vRendererCuda::render, src/vRendererCuda.cpp:107-165).  After a call of one
 * launch on the context stream (one frame per call, the reference's cadence)
 * it returns as soon as the finish pass's last block has stored its results:
 * the pass counts its blocks' arrivals and the last one stores the call's
 * number to host-coherent memory, which vrhip_sync polls -- about 8 us
 * before the stream's own completion signal reaches the host.  Work the
 * library or the caller queues on the context stream afterwards is ordered
 * behind the pass as usual.  A context whose stream or buffers were handed
 * out (vrhip_get_stream, vrhip_set_stream, vrhip_device_buffers: the caller
 * may read the images from its own streams) always waits for the stream, as
 * does a context with a communicator.  vrhip_set_sync_flag(ctx, 0), or
 * VRHIP_SYNC_FLAG=0 in the environment at creation, turns the flag off. */
int vrhip_sync(vrhip_ctx *ctx);
int vrhip_set_sync_flag(vrhip_ctx *ctx, int on);
/* Synchronisations since the context was created (diagnostics): out[0] ended
 * by the completion flag, out[1] by waiting for the stream. */
#define VRHIP_SYNC_INFO 2
int vrhip_sync_info(vrhip_ctx *ctx, uint64_t out[VRHIP_SYNC_INFO]);
/* Path groups per pixel for vrhip_render in sphere-only scenes (no
 * reference counterpart: a launch shape knob; mesh scenes use the persistent
 * path kernel, whose work queues need none).  A launch of k frames has 2k
 * paths per pixel; with groups > 1 they are split into that many contiguous
 * runs on different workgroups and summed in path order afterwards, so
 * results are unchanged.  0 (default) picks the smallest power of two that
 * gives every CU enough workgroups; 1 disables the split.  At most 128. */
int vrhip_set_path_split(vrhip_ctx *ctx, uint32_t groups);
/* Overlap of consecutive render launches (no reference counterpart: a
 * scheduling knob; results are unchanged).  The path kernels of launch i+1
 * may start on another of three internal path streams while launch i drains
 * its last paths; finish passes (accumulation, tonemap) stay in order on the
 * context stream, and any upload, tiling or stream change first waits for
 * the path streams.  mode 1: always, 0: never (launches run one after the
 * other), -1 (default): when a launch has fewer than 2^24 paths, or fewer
 * than 2^25 on a tiled rank (small or sharded frames, where the drain of a
 * launch is a large share of it). */
int vrhip_set_overlap(vrhip_ctx *ctx, int mode);
/* Render service (no reference counterpart: a scheduling mode; results are
 * unchanged bit for bit).  Consecutive vrhip_render calls of a mesh scene run
 * as one session on ONE persistent kernel: each launch is posted to a
 * descriptor ring the running kernel reads, so the drain of a launch (its
 * last, longest paths) overlaps the next launch's paths instead of ending a
 * kernel.  The images are summed, in path order, by one finish pass when the
 * session closes: at the next call on the context that is not vrhip_render or
 * vrhip_comm_gather (sync, read-back, upload, any setting, ...), when its 128
 * launch slots are used, or when a launch does not fit it (another scene,
 * camera or tiling, more frames than its slots hold).  vrhip_comm_gather
 * inside a session gathers the image as of that call when the session closes.
 * mode 1: every production mesh launch; 0: never; -1 (default, also
 * VRHIP_SERVICE): launches that overlap on the path streams (fewer than 2^24
 * paths, or 2^25 on a tiled rank) when the previous launch is still in flight
 * -- unsynchronised back-to-back calls, not the first call of a burst; also
 * whole frames of HDRI mesh scenes behind a launch in flight.  Launches whose
 * result slots the service's scratch budget (VRHIP_SERVICE_BYTES, default 24
 * GiB; a session's slots also take at most half of the device memory free when
 * it opens) cannot hold twice take the ordinary launch path in every mode, as
 * do the launches of a session whose scratch allocation fails.  The
 * open session's kernel retires after 20 ms without a new launch; a launch
 * posted while it retires is detected (a store-fence-load hand-shake on the
 * ring) and rendered through the launch path instead.
 * Gathers (vrhip_comm_gather) inside a session:
 *   mode -1 (automatic): the gather closes the session and is enqueued at
 *   once, like outside a session -- no collective ever waits on a later host
 *   call, whatever the caller does next.
 *   mode 1 (explicit): the gather is DEFERRED -- the image as of that call is
 *   staged by the session's finish pass and its ncclGather enqueued when the
 *   session closes, so consecutive steps keep one session (their drains
 *   overlap).  The caller then owns the ordering: a rank must close its
 *   session before it blocks on anything the other ranks' gathers wait for
 *   (a host barrier, a device-wide synchronise).  Calls that close a session:
 *   vrhip_sync, vrhip_read_accum/rgba8/depth8, vrhip_device_buffers,
 *   vrhip_gl_present, vrhip_pack_tiles/unpack_tiles, vrhip_last_kernel_ms,
 *   vrhip_kernel_stats, vrhip_debug_counters, vrhip_set_camera, vrhip_clear,
 *   every upload (vrhip_upload_mesh_device too), vrhip_refit_mesh_device,
 *   vrhip_bvh_sah_cost, vrhip_export_mesh_flat, vrhip_trace_rays, vrhip_trace_radiance, vrhip_trace_surface, vrhip_shade_surface, vrhip_probe_sh, vrhip_sh_irradiance, vrhip_camera_rays, vrhip_surface_at, vrhip_atlas_surface, vrhip_denoise, vrhip_denoise_frame, vrhip_set_stream, vrhip_set_tiling, vrhip_set_service
 *   (and its timing / budget hooks), vrhip_comm_init/destroy, vrhip_destroy,
 *   the counting renders, and a vrhip_render that does not fit the session.
 *   Calls that do NOT close it: the flag setters (Cornell box, example sphere,
 *   BRDF, strict traversal, Fresnel -- the next vrhip_render then no longer
 *   fits and closes it), vrhip_set_overlap, vrhip_set_path_split,
 *   vrhip_set_kernel_timing, and the queries vrhip_frame_count,
 *   vrhip_last_launch_info, vrhip_owned_pixels, vrhip_service_stats/info,
 *   vrhip_device_group, vrhip_bvh_info, vrhip_get_stream. */
int vrhip_set_service(vrhip_ctx *ctx, int mode);
/* Render-service timing (test hook, no reference counterpart; 0 = default):
 * the session kernel's idle limit (20 ms), the host's window for posting to
 * an open session after its last post (5 ms), and a host delay inserted
 * between that window check and the post -- with a delay longer than the idle
 * limit every post after a session's first meets a retired kernel, which
 * exercises the hand-shake above.  Each at most 10 s. */
int vrhip_set_service_timing(vrhip_ctx *ctx, uint32_t idle_us, uint32_t post_window_us, uint32_t post_delay_us);
/* Scratch budget of the render service's launch slots on this context
 * (bytes; 0 = VRHIP_SERVICE_BYTES or 24 GiB).  A launch whose slot the budget
 * cannot hold twice takes the ordinary launch path. */
int vrhip_set_service_budget(vrhip_ctx *ctx, size_t bytes);
/* Launches that met a retiring session kernel and took the launch path
 * instead (since the context was created). */
int vrhip_service_stats(vrhip_ctx *ctx, uint64_t *refused_launches);
/* Render-service counts since the context was created (diagnostics; no
 * reference counterpart): out[0] launches refused by a retiring kernel (as
 * vrhip_service_stats), [1] sessions opened, [2] launches sessions took,
 * [3] gathers deferred to a session's close (explicit mode 1 only), [4]
 * sessions not opened because their scratch could not be allocated (those
 * launches took the launch path). */
#define VRHIP_SERVICE_INFO 5
int vrhip_service_info(vrhip_ctx *ctx, uint64_t out[VRHIP_SERVICE_INFO]);
/* Frames rendered since the last clear (vRendererCuda::getFrameCount,
 * include/vRendererCuda.h:124). */
int vrhip_frame_count(vrhip_ctx *ctx, uint32_t *frames);

/* ---- read-back -------------------------------------------------------- */
int vrhip_read_accum(vrhip_ctx *ctx, float *out_rgba_f32);       /* float4[W*H] */
int vrhip_read_rgba8(vrhip_ctx *ctx, uint8_t *out_rgba8);        /* uchar4[W*H] */
int vrhip_read_depth8(vrhip_ctx *ctx, uint8_t *out_rgba8);       /* uchar4[W*H] */
/* Device pointers of the resident buffers (for GL interop / RCCL gather). */
int vrhip_device_buffers(vrhip_ctx *ctx, void **accum, void **rgba8, void **depth8);

/* ---- multi-GPU image-tile sharding ------------------------------------ */
/* Render only the 16x16 tiles dealt to `rank`: rank r holds the tiles at
 * positions s = r, r + n_ranks, r + 2 n_ranks, ... of the dealing sequence,
 * and position s is the tile in row s / tiles_x, column
 * (s % tiles_x + s / tiles_x) % tiles_x (tiles_x = width / 16; each row
 * rotated by its index, ABI 5 -- ABI 4 dealt row-major, which gives every
 * rank fixed columns when tiles_x is a multiple of n_ranks); with
 * n_ranks == 1 the order stays row-major.  Every rank gets
 * the same number of tiles (+-1) spread over the whole image.
 * Seeds use global pixel coordinates, so the union of the ranks' tiles equals
 * the 1-GPU image bit for bit.  VRHIP_ERR_INVALID while a communicator
 * (vrhip_comm_init) with another tiling exists. */
int vrhip_set_tiling(vrhip_ctx *ctx, uint32_t rank, uint32_t n_ranks);
/* Host-only (no device): linear pixel indices (y * width + x) that rank
 * `rank` of n_ranks owns, in packed order (owned tile j holds packed pixels
 * [256j, 256j + 256), row-major inside the tile).  pix_out may be NULL to
 * query *n_pix. */
int vrhip_tile_pixels(uint32_t width, uint32_t height, uint32_t rank, uint32_t n_ranks, uint32_t *pix_out,
                      uint32_t *n_pix);
/* Number of pixels this rank owns (256 per owned tile). */
int vrhip_owned_pixels(vrhip_ctx *ctx, uint32_t *n_pix);
/* Pack this rank's owned pixels (RGBA8 if what == 0, float4 accum if 1,
 * depth8 if 2) contiguously into dst (device pointer), in packed order. */
int vrhip_pack_tiles(vrhip_ctx *ctx, int what, void *dst_device);
/* On the gathering rank: scatter n_ranks packed buffers from src (device;
 * rank r's buffer starts at r * stride_bytes, stride_bytes = 0 means
 * tightly packed) into this context's full image `what`. */
int vrhip_unpack_tiles(vrhip_ctx *ctx, int what, const void *src_device, uint32_t n_ranks, size_t stride_bytes);

/* ---- multi-GPU tile gather over RCCL (xGMI) ----------------------------- */
/* The reference is single-GPU; its per-pixel seeds use global pixel
 * coordinates (cuda/src/PathTracer.cu:817-818), so ranks rendering disjoint
 * tile sets reproduce the 1-GPU image bit for bit.  One process (or thread)
 * per GPU, one context per rank:
 *   rank 0: vrhip_comm_unique_id(id); hand `id` to every rank out of band
 *   (MPI, a file, a socket, torch.distributed ...);
 *   every rank: vrhip_comm_init(ctx, rank, n, id) -- joins the communicator
 *   (ncclCommInitRank: blocks until all n ranks have called it) and sets the
 *   tiling (vrhip_set_tiling(ctx, rank, n));
 *   per accumulation step, after vrhip_render: vrhip_comm_gather(ctx, what).
 * VRHIP_COMM_ID_BYTES = sizeof(ncclUniqueId). */
#define VRHIP_COMM_ID_BYTES 128
int vrhip_comm_unique_id(uint8_t id[VRHIP_COMM_ID_BYTES]);
int vrhip_comm_init(vrhip_ctx *ctx, uint32_t rank, uint32_t n_ranks, const uint8_t id[VRHIP_COMM_ID_BYTES]);
/* Every rank packs its tiles of image `what` (0 RGBA8, 1 float4 accumulation,
 * 2 depth8), ONE ncclGather brings them to rank 0, and rank 0 scatters them
 * into its full image -- all enqueued on the context stream behind the
 * render's finish passes (no host synchronisation).  Rank 0's image `what`
 * then holds the whole frame.  Inside a render-service session it closes the
 * session first (automatic service mode, the default), or, in explicit
 * service mode 1, is deferred to the session's close -- then call vrhip_sync
 * before any host-side barrier between ranks (vrhip_set_service). */
int vrhip_comm_gather(vrhip_ctx *ctx, int what);
/* Leaves the communicator (waits for the context stream first).  vrhip_destroy does it too. */
int vrhip_comm_destroy(vrhip_ctx *ctx);

/* ---- diagnostics ------------------------------------------------------ */
/* Kernel time of the last vrhip_render (ms, HIP events on the context stream;
 * requires vrhip_sync first; 0 with kernel timing off).  After a
 * render-service session: the session's span, from its kernel's start to its
 * finish pass's end (all its launches). */
int vrhip_last_kernel_ms(vrhip_ctx *ctx, float *ms);
/* Kernel timing (diagnostics; no reference counterpart): on (default; also
 * VRHIP_KERNEL_TIMING=1) the library records HIP events around each call and
 * around every launch's render kernels for vrhip_last_kernel_ms and
 * vrhip_kernel_stats; off, it records none on the launch path -- they sit
 * between the kernels on the stream and cost about 8 µs per synchronous
 * one-frame call (C2 0.712 -> 0.704 ms per frame), so a host at the
 * reference's one-frame cadence that does not read them turns them off. */
int vrhip_set_kernel_timing(vrhip_ctx *ctx, int on);
/* Accumulated render-kernel time (ms) and launch count since the last reset,
 * from HIP events recorded around every launch's render kernels
 * (primary_kernel + render_wave_kernel, or render_kernel) on the stream they
 * run on; the finish pass is not included.  With launch overlap a launch's
 * span includes time shared with the neighbouring launch.  Waits for the
 * pending launches. */
int vrhip_kernel_stats(vrhip_ctx *ctx, double *total_ms, uint64_t *launches, int reset);
/* Shape of the last production launch of vrhip_render (measurement; no
 * reference counterpart): path groups per pixel (sphere-only scenes), whether
 * the paths' results went through the result scratch and the finish pass (1)
 * or were accumulated in registers in path order (0), and the kernel family
 * (0 render_kernel, 1 path-pool kernel, 2 render service, 3 path-pool kernel
 * + finish pass as one graph launch: VRHIP_GRAPH=1, one-frame calls). */
int vrhip_last_launch_info(vrhip_ctx *ctx, uint32_t *split, uint32_t *use_scratch, uint32_t *kind);
/* Vector-memory gather roof of `device` (the ceiling the path kernel's
 * node, triangle and attribute fetches run against; no reference
 * counterpart): raw buffer loads of width_bytes (4, 8, 12 or 16) per lane
 * from a 1 MiB L2-resident table, 4 independent chains per lane, 8 waves per
 * SIMD on every CU, the 64 lanes of a wave reading `distinct` addresses
 * (1: one per wave-instruction ... 64: one per lane).  *lane_loads_per_s =
 * lane loads (one per active lane per instruction) per second, best of 3
 * warm launches.  Synchronous; a few ms. */
int vrhip_microbench_vmem(int device, uint32_t width_bytes, uint32_t distinct, double *lane_loads_per_s);
/* Raw debug slots: [0..7] the last counted render's counters; [8..13] phase
 * cycle totals (spheres, mesh traversal, hit materialisation, shading,
 * tonemap, whole kernel) written only by a -DVR_TIMING diagnostic build. */
int vrhip_debug_counters(vrhip_ctx *ctx, uint64_t out[16], int reset);
/* Depth of the uploaded BVH and the traversal stack size in use. */
int vrhip_bvh_info(vrhip_ctx *ctx, uint32_t *depth, uint32_t *n_nodes, uint32_t *n_slots);
/* Evaluate the device libm on n inputs (test hook); a, b, out host arrays of n
 * floats (b is read only by the binary functions but must not be NULL).  fn:
 *    0 sin(a)   1 cos(a)   2 acos(a)   3 atan2(a, b)   4 pow(a, b)
 *    5 fmin(a, b)   6 fmax(a, b)
 *    7 f2i(a): float -> int, truncating, saturating, NaN -> 0; the int's bits
 *    8 d2i((double)a * (double)b): the same from double; the int's bits
 *    9 f2u8(a): the colour byte (truncate, clamp to [0, 255], NaN -> 0) as a
 *      float value
 *   10 sqrt_exact(a)   11 inv_sqrt_exact(a): the path kernels' sqrtf(a) and
 *      1.0f / sqrtf(a), which take a short sequence when every lane of the
 *      wave is inside its exact range and the IEEE expansion otherwise
 *   any other value writes 0.
 * fn | 0x100 (fn 0..4) runs the same function as compiled in the other of the
 * two constant forms of the device libm: the one the sphere-only kernels use
 * (constants the compiler may hoist) instead of the one the mesh kernels use
 * (constants materialised at each use); VRHIP_ERR_INVALID for fn > 4.
 * Lane mapping: element i is thread i of a one-dimensional grid of 256-thread
 * blocks, so lane i % 64 of wave i / 64; the layout of a therefore decides
 * which values share a wave in fn 10 and 11, and a last wave of n % 64
 * elements votes over those lanes only.  n == 0 launches nothing and is
 * VRHIP_OK.  The device buffers are freed on every return. */
int vrhip_selftest_math(int device, int fn, const float *a, const float *b, float *out, size_t n);
/* The BRDF lookup of the shading step (lookupBRDF, PathTracer.cu:519-566) on
 * n caller-supplied frames (test hook).  table: a planar MERL table as
 * vrhip_upload_brdf takes it, n_floats == 3*90*90*180 (anything else is
 * VRHIP_ERR_INVALID), interleaved and uploaded as vrhip_upload_brdf does.
 * frames: 16 n floats, per frame the float4s refl (the sampled direction),
 * cur (the arriving ray's direction), normal, tangent; nothing is normalised
 * or checked: the three table indices are clamped, so no input reads outside
 * the table.  out: 4 n floats, the lookup's float4 (r/1500, g*1.15/1500,
 * b*1.66/1500, 0) per frame, before the shading step's max with 0. */
int vrhip_selftest_brdf(int device, const float *table, size_t n_floats, const float *frames, size_t n, float *out);
/* The device BVH builder's outward fp32 -> fp16 box rounding on n host
 * floats (test hook): down[i] rounded toward -inf, up[i] toward +inf, as
 * binary16 bit patterns. */
int vrhip_selftest_half_box(int device, const float *in, size_t n, uint16_t *down, uint16_t *up);
/* Compare the kernels' reciprocal (rcp_rn: v_rcp_f32 + one Newton step, used
 * for 1/det in the triangle test) with IEEE 1/x for every float bit pattern in
 * [lo_bits, hi_bits) and its negation (test hook; hi_bits <= 2^31).
 * *mismatches = count, *first_bad = smallest mismatching pattern or ~0u. */
int vrhip_selftest_rcp(int device, uint32_t lo_bits, uint32_t hi_bits, uint64_t *mismatches, uint32_t *first_bad);
/* The same for the kernels' square root (sqrt_rn: v_sqrt_f32 + the neighbour
 * tests of the IEEE expansion) against sqrtf, positive patterns only. */
int vrhip_selftest_sqrt(int device, uint32_t lo_bits, uint32_t hi_bits, uint64_t *mismatches, uint32_t *first_bad);
/* Exhaustive check of the table tonemap (no reference counterpart): the
 * colour byte the kernels take from the context's threshold table against
 * the byte of f2u8(pow(c, 1/2.2) * 255) (PathTracer.cu:850-866, the f64
 * pow), for every float bit pattern c in [lo_bits, hi_bits) (and -0.0 when
 * lo_bits is 0); the range [0, 0x3f800001) is every clamped channel value. */
int vrhip_selftest_tonemap(int device, uint32_t lo_bits, uint32_t hi_bits, uint64_t *mismatches, uint32_t *first_bad);

/* ---- host-side helpers (no device needed) ----------------------------- */
/* Native BVH build + reference flattening (src/vRendererCuda.cpp:204-279)
 * into caller arrays.  Call once with NULL outputs to get the sizes. */
int vrhip_build_flat(const float *positions, const float *normals, const float *tangents,
                     const float *uvs, uint32_t n_verts, const uint32_t *tris, uint32_t n_tris,
                     uint32_t max_leaf_tris,
                     float *bvh_out, size_t *n_bvh_f4,
                     float *verts_out, float *normals_out, float *tangents_out, float *uvs_out,
                     size_t *n_slots);
/* Check a flattened tree; returns VRHIP_OK and its depth / inner-node count. */
int vrhip_validate_flat(const float *bvh, size_t n_bvh_f4, const float *verts, size_t n_slots,
                        uint32_t *depth, uint32_t *n_nodes);
/* vrhip_bvh_sah_cost's definition evaluated on the host over a flattened tree
 * (checked first as vrhip_validate_flat does: VRHIP_ERR_BVH if malformed); a
 * leaf's triangle count is its run of triples up to the terminator.  The
 * yardstick for the device value, and the cost of a cached tree without a GPU. */
int vrhip_flat_sah_cost(const float *bvh, size_t n_bvh_f4, const float *verts, size_t n_slots,
                        double *cost);
/* vrhip_trace_rays on the host over a flattened tree, host pointers throughout
 * (checked first as vrhip_validate_flat does: VRHIP_ERR_BVH if malformed;
 * VRHIP_ERR_INVALID for null arrays or an unknown mode): one lane of the
 * reference's walk (cuda/src/PathTracer.cu:276-463) -- every pierced box, near
 * child first and child 0 on equal entries, leaf slots in order up to the
 * terminator, strict < on the closest-hit update.  Same records and semantics;
 * `prim` is the slot of the hit triangle's first vertex.  The yardstick for the
 * device query, and ray queries on a cached tree without a GPU. */
int vrhip_flat_trace_rays(const float *bvh, size_t n_bvh_f4, const float *verts, size_t n_slots,
                          const float *origins, const float *dirs, const float *tmax, uint32_t n_rays,
                          uint32_t mode, vrhip_ray_hit *hits);

#ifdef __cplusplus
}
#endif
#endif /* VRHIP_H */
