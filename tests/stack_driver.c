/* TEST INFRASTRUCTURE ONLY -- the oracle with a traversal stack of a settable
 * size, for the mutants of tests/test_stack_cpu.py.
 *
 * This file includes oracle/vro.c with the two macros that no build of the
 * oracle defines: the stack's capacity is a variable (64 until set), and a
 * push that finds the stack full is lost instead of being error -3.  With the
 * capacity at a tree's depth + 1 every push fits and the render is the
 * oracle's own, bit for bit; one entry fewer loses the last push of every ray
 * that fills its stack, which is what an off-by-one in a kernel's stack size or
 * indexing would do to it.  Compiled by tests/stack_cases.py into a shared
 * object of its own with oracle/Makefile's CFLAGS, plus vro_math.c; nothing in
 * the product links it.
 *
 * vro_render of this object is the mutant render.  stack_driver_rays is
 * intersect_scene on arbitrary rays, called as tests/surface_driver.c calls it
 * (the direction normalised by normalize4: the sphere tests need that), and
 * returns each ray's largest stack pointer as well.
 */
static int stack_capacity = 64;
#define VRO_STACK_CAPACITY stack_capacity
#define VRO_STACK_DROP 1
#include "vro.c"

/* entries the stack holds, the sentinel's included: 1 .. VRO_STACK_ENTRIES */
int stack_driver_capacity(int entries)
{
    if (entries < 1 || entries > VRO_STACK_ENTRIES) return -1;
    stack_capacity = entries;
    return 0;
}

/* origins, dirs: float[3 n].  hits: float[24 n], rows hitPoint, normal,
 * tangent, emission, color, spec as float4.  types, hit, high_water: [n].
 * Returns tctx.err. */
int stack_driver_rays(const vro_scene *sc, const float *origins, const float *dirs, uint32_t n, float *hits,
                      uint32_t *types, int32_t *hit, uint32_t *high_water)
{
    tctx tc;
    memset(&tc, 0, sizeof(tc));
    tc.sc = sc;
    tc.m.libm = sc->libm;
    for (uint32_t i = 0; i < n; ++i) {
        vro_counters cnt;
        memset(&cnt, 0, sizeof(cnt));
        tc.cnt = &cnt;
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
        high_water[i] = (uint32_t)cnt.max_stack;
    }
    return tc.err;
}
