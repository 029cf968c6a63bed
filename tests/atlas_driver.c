/* TEST INFRASTRUCTURE ONLY -- the yardstick of vrhip_surface_at and
 * vrhip_atlas_surface.
 *
 * This file includes oracle/vro.c, so the leaf_hit called here is the static
 * function the reference-rendered fixtures pin through the renders.  Compiled
 * by tests/atlas_cases.py into a shared object of its own with oracle/Makefile's
 * CFLAGS (-ffp-contract=off among them), plus vro_math.c; nothing in the
 * product links it.
 *
 * atlas_at      the record at (slot, u, v): leaf_hit with I = (0, u, v) and a
 *               ray of zeros, the hit point then overwritten with the
 *               barycentric position; kind, prim, the barycentrics and the
 *               interpolated uv restated as tests/surface_cases.py restates them.
 * atlas_raster  the definition in include/vrhip.h in plain C, brute force over
 *               all triangles per texel, or (use_box) triangle by triangle over
 *               a bounding box of its own; then the gutter passes; then atlas_at
 *               per texel.
 * A record is 28 uint32 words in the order of vrhip_surface_hit.
 */
#include "vro.c"

static uint32_t fb(float f) { return fbits(f); }

/* is_first[i]: slot i is the first vertex of a triangle (the scan of
 * intersect_scene's brute-force mode, vro.c) */
void atlas_first_slots(const vro_scene *sc, uint8_t *is_first)
{
    memset(is_first, 0, sc->n_slots);
    size_t i = 0;
    while (i < sc->n_slots) {
        if (fbits(sc->verts[4 * i]) == 0x80000000u) { i += 1; continue; }
        is_first[i] = 1;
        i += 3;
    }
}

static void record_at(const vro_scene *sc, uint32_t slot, uint32_t prim, float u, float v, float t, uint32_t *rec)
{
    tctx tc;
    memset(&tc, 0, sizeof(tc));
    tc.sc = sc;
    tc.m.libm = sc->libm;
    ray_t r;
    memset(&r, 0, sizeof(r));
    hit_t h;
    memset(&h, 0, sizeof(h));
    vf4 v0 = ld4(sc->verts, slot), v1 = ld4(sc->verts, slot + 1), v2 = ld4(sc->verts, slot + 2);
    float tt = 0.f;
    leaf_hit(&tc, &r, (int)slot, v0, v1, v2, f4(0.f, u, v, 0.f), &tt, &h);
    float b0 = 1.0f - u - v;
    float px = (b0 * v0.x + u * v1.x) + v * v2.x;
    float py = (b0 * v0.y + u * v1.y) + v * v2.y;
    float pz = (b0 * v0.z + u * v1.z) + v * v2.z;
    vf2 uv0 = ld2(sc->uvs, slot), uv1 = ld2(sc->uvs, slot + 1), uv2 = ld2(sc->uvs, slot + 2);
    float tu = (b0 * uv0.x + u * uv1.x) + v * uv2.x;
    float tv = (b0 * uv0.y + u * uv1.y) + v * uv2.y;
    const uint32_t w[28] = {
        fb(t), 4u, prim, h.hitType,
        fb(px), fb(py), fb(pz), fb(u),
        fb(h.normal.x), fb(h.normal.y), fb(h.normal.z), fb(v),
        fb(h.tangent.x), fb(h.tangent.y), fb(h.tangent.z), 0u,
        fb(h.color.x), fb(h.color.y), fb(h.color.z), fb(tu),
        fb(h.spec.x), fb(h.spec.y), fb(h.spec.z), fb(tv),
        fb(h.emission.x), fb(h.emission.y), fb(h.emission.z), 0u };
    memcpy(rec, w, sizeof(w));
}

static int finite_f(float f) { return (fbits(f) & 0x7f800000u) != 0x7f800000u; }

/* slots, bary [2n] -> recs [28 n]; an entry whose slot is no triangle's first
 * vertex or whose u or v is not finite: 28 zero words. */
void atlas_at(const vro_scene *sc, const uint32_t *slots, const float *bary, uint32_t n, uint32_t *recs)
{
    uint8_t *first = (uint8_t *)malloc(sc->n_slots ? sc->n_slots : 1);
    atlas_first_slots(sc, first);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t *rec = recs + 28 * (size_t)i;
        memset(rec, 0, 28 * sizeof(uint32_t));
        float u = bary[2 * i], v = bary[2 * i + 1];
        if ((size_t)slots[i] >= sc->n_slots || !first[slots[i]] || !finite_f(u) || !finite_f(v)) continue;
        record_at(sc, slots[i], slots[i], u, v, 0.f, rec);
    }
    free(first);
}

int atlas_tex_addr(uint32_t w, uint32_t h, float u, float v) { return tex_addr(w, h, u, v); }

/* ---- the raster ---- */
typedef struct { double ax, ay, bx, by, cx, cy, A2; int ok; } tri_uv;

static double edge_canon(double px, double py, double qx, double qy, double x, double y)
{
    int sw = qx < px || (qx == px && qy < py);
    if (sw) { double t = px; px = qx; qx = t; t = py; py = qy; qy = t; }
    double e = (qx - px) * (y - py) - (qy - py) * (x - px);
    return sw ? -e : e;
}

static int finite_d(double d) { return d - d == 0.0; }

static tri_uv tri_of(const vro_scene *sc, size_t slot)
{
    tri_uv t;
    vf2 a = ld2(sc->uvs, slot), b = ld2(sc->uvs, slot + 1), c = ld2(sc->uvs, slot + 2);
    t.ax = a.x; t.ay = a.y; t.bx = b.x; t.by = b.y; t.cx = c.x; t.cy = c.y;
    t.ok = finite_f(a.x) && finite_f(a.y) && finite_f(b.x) && finite_f(b.y) && finite_f(c.x) && finite_f(c.y);
    t.A2 = 0.0;
    if (t.ok) {
        t.A2 = edge_canon(t.ax, t.ay, t.bx, t.by, t.cx, t.cy);
        t.ok = t.A2 != 0.0 && finite_d(t.A2);
    }
    return t;
}

static int covers(const tri_uv *t, double x, double y)
{
    double e0 = edge_canon(t->ax, t->ay, t->bx, t->by, x, y);
    double e1 = edge_canon(t->bx, t->by, t->cx, t->cy, x, y);
    double e2 = edge_canon(t->cx, t->cy, t->ax, t->ay, x, y);
    return t->A2 > 0.0 ? (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) : (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
}

typedef struct { uint32_t slot, prim, dist; float u, v; } cell_t;
#define NONE 0xffffffffu

static double min3(double a, double b, double c) { double m = a < b ? a : b; return m < c ? m : c; }
static double max3(double a, double b, double c) { double m = a > b ? a : b; return m > c ? m : c; }

/* the texels of one axis a triangle spanning [mn, mx] can cover, generously:
 * two texels of slack on either side, clipped while still a double */
static int axis_range(double mn, double mx, uint32_t n, uint32_t *lo, uint32_t *hi)
{
    double l = mn * (double)n - 2.5, h = mx * (double)n + 2.5;
    if (h < 0.0 || l > (double)(n - 1)) return 0;
    *lo = l <= 0.0 ? 0u : (uint32_t)l;
    *hi = h >= (double)(n - 1) ? n - 1 : (uint32_t)h;
    return 1;
}

/* prim_of_slot: the caller's name of the triangle whose first vertex is each
 * slot, or NULL for the slot itself.  recs: [28 W H]. */
void atlas_raster(const vro_scene *sc, const uint32_t *prim_of_slot, uint32_t W, uint32_t H, uint32_t gutter, int use_box,
                  uint32_t *recs)
{
    size_t n = (size_t)W * H;
    cell_t *cell = (cell_t *)malloc(n * sizeof(cell_t)), *next = (cell_t *)malloc(n * sizeof(cell_t));
    uint8_t *first = (uint8_t *)malloc(sc->n_slots ? sc->n_slots : 1);
    atlas_first_slots(sc, first);
    for (size_t i = 0; i < n; ++i) { cell[i].slot = NONE; cell[i].prim = NONE; cell[i].dist = 0; cell[i].u = cell[i].v = 0.f; }
    for (size_t s = 0; s < sc->n_slots; ++s) {
        if (!first[s]) continue;
        tri_uv t = tri_of(sc, s);
        if (!t.ok) continue;
        uint32_t prim = prim_of_slot ? prim_of_slot[s] : (uint32_t)s;
        uint32_t x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;
        if (use_box && (!axis_range(min3(t.ax, t.bx, t.cx), max3(t.ax, t.bx, t.cx), W, &x0, &x1) ||
                        !axis_range(min3(t.ay, t.by, t.cy), max3(t.ay, t.by, t.cy), H, &y0, &y1)))
            continue;
        for (uint32_t y = y0; y <= y1; ++y)
            for (uint32_t x = x0; x <= x1; ++x) {
                double cx = ((double)x + 0.5) / (double)W, cy = ((double)y + 0.5) / (double)H;
                cell_t *c = &cell[(size_t)y * W + x];
                /* the smallest prim; between two stored copies of one prim, the first stored */
                if (covers(&t, cx, cy) && (prim < c->prim || (c->slot == NONE))) { c->prim = prim; c->slot = (uint32_t)s; }
            }
    }
    for (size_t i = 0; i < n; ++i) {
        cell_t *c = &cell[i];
        if (c->slot == NONE) continue;
        tri_uv t = tri_of(sc, c->slot);
        double cx = ((double)(i % W) + 0.5) / (double)W, cy = ((double)(i / W) + 0.5) / (double)H;
        double eu = (cx - t.ax) * (t.cy - t.ay) - (cy - t.ay) * (t.cx - t.ax);
        double ev = (t.bx - t.ax) * (cy - t.ay) - (t.by - t.ay) * (cx - t.ax);
        double ud = eu / t.A2, vd = ev / t.A2;
        ud = ud < 0.0 ? 0.0 : ud > 1.0 ? 1.0 : ud;
        vd = vd < 0.0 ? 0.0 : vd > 1.0 ? 1.0 : vd;
        c->u = (float)ud; c->v = (float)vd;
        if (c->u + c->v > 1.f) c->v = 1.f - c->u;
    }
    static const int dx[8] = { -1, 1, 0, 0, -1, 1, -1, 1 }, dy[8] = { 0, 0, -1, 1, -1, -1, 1, 1 };
    for (uint32_t k = 1; k <= gutter; ++k) {
        for (size_t i = 0; i < n; ++i) {
            next[i] = cell[i];
            if (cell[i].slot != NONE) continue;
            long x = (long)(i % W), y = (long)(i / W);
            for (int j = 0; j < 8; ++j) {
                long nx = x + dx[j], ny = y + dy[j];
                if (nx < 0 || ny < 0 || nx >= (long)W || ny >= (long)H) continue;
                const cell_t *nb = &cell[(size_t)ny * W + (size_t)nx];
                if (nb->slot != NONE) { next[i] = *nb; next[i].dist = k; break; }
            }
        }
        cell_t *tmp = cell; cell = next; next = tmp;
    }
    for (size_t i = 0; i < n; ++i) {
        uint32_t *rec = recs + 28 * i;
        memset(rec, 0, 28 * sizeof(uint32_t));
        if (cell[i].slot == NONE) { rec[0] = fb(1e20f); rec[2] = NONE; continue; }
        record_at(sc, cell[i].slot, cell[i].prim, cell[i].u, cell[i].v, (float)cell[i].dist, rec);
    }
    free(first); free(cell); free(next);
}
