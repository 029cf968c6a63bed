/* TEST INFRASTRUCTURE ONLY -- the yardstick of vrhip_trace_surface.
 *
 * The oracle's own intersect_scene (oracle/vro.c, static) on arbitrary rays:
 * this file includes vro.c, so the function called here is the one the
 * reference-rendered fixtures pin through the renders.  Compiled by
 * tests/surface_cases.py into a shared object of its own with oracle/Makefile's
 * CFLAGS, plus vro_math.c; nothing in the product links it.
 *
 * Per ray: a hit_t of zeros (as trace starts, vro.c trace), the direction
 * normalised by normalize4 (as primary_ray does), intersect_scene in the
 * scene's libm mode.  Beside the hit_t fields it returns which sphere is the
 * closest and at what t: a restatement of the selection loops of
 * intersect_scene (vro.c:298-311: dist != 0 && dist < t, same order) over the
 * oracle's own sphere_intersect.  The mesh part of (kind, index, t) is added by
 * surface_cases.py.
 */
#include "vro.c"

enum { SD_NONE = 0, SD_CORNELL = 1, SD_SMALL = 2, SD_EXAMPLE = 3 };

/* origins, dirs: float[3 n].  hits: float[24 n], rows hitPoint, normal,
 * tangent, emission, color, spec as float4.  types, hit, kind, index: [n].
 * sphere_t: float[n], 1e20 when no sphere is hit.  Returns tctx.err. */
int surface_driver(const vro_scene *sc, const float *origins, const float *dirs, uint32_t n, float *hits,
                   uint32_t *types, int32_t *hit, int32_t *kind, int32_t *index, float *sphere_t)
{
    tctx tc;
    memset(&tc, 0, sizeof(tc));
    tc.sc = sc;
    tc.m.libm = sc->libm;
    for (uint32_t i = 0; i < n; ++i) {
        ray_t r;
        r.o = f4(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], 0.f);
        r.d = normalize4(f4(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], 0.f));
        hit_t h;
        memset(&h, 0, sizeof(h));
        hit[i] = intersect_scene(&tc, &r, &h);
        const vf4 rows[6] = { h.hitPoint, h.normal, h.tangent, h.emission, h.color, h.spec };
        for (int k = 0; k < 6; ++k) {
            float *o = hits + 24 * (size_t)i + 4 * k;
            o[0] = rows[k].x; o[1] = rows[k].y; o[2] = rows[k].z; o[3] = rows[k].w;
        }
        types[i] = h.hitType;

        float t = 1e20f;
        int kd = SD_NONE, ix = 0;
        if (sc->use_cornell) {
            for (int s = 0; s < 6; ++s) {
                float dist = sphere_intersect(&k_cornell[s], &r);
                if (dist != 0.f && dist < t) { t = dist; kd = SD_CORNELL; ix = s; }
            }
        }
        for (int s = 0; s < 2; ++s) {
            float dist = sphere_intersect(&k_spheres[s], &r);
            if (dist != 0.f && dist < t) { t = dist; kd = SD_SMALL; ix = s; }
        }
        if (sc->use_example_sphere) {
            float dist = sphere_intersect(&k_example, &r);
            if (dist != 0.f && dist < t) { t = dist; kd = SD_EXAMPLE; ix = 0; }
        }
        kind[i] = kd; index[i] = ix; sphere_t[i] = t;
    }
    return tc.err;
}

/* Colour and emission of a sphere by (kind, index), for the test that ties the
 * restated selection to the records. */
void surface_driver_sphere(int kind, int index, float *color3, float *emission3)
{
    const sphere_t *s = kind == SD_CORNELL ? &k_cornell[index] : kind == SD_SMALL ? &k_spheres[index] : &k_example;
    color3[0] = s->col.x; color3[1] = s->col.y; color3[2] = s->col.z;
    emission3[0] = s->emission.x; emission3[1] = s->emission.y; emission3[2] = s->emission.z;
}
