// vr_denoise.hip -- the edge-avoiding a-trous filter (vr_denoise.hpp; the
// definition: include/vrhip.h, vrhip_denoise).  Three kernels:
//   prep    reads each 112-byte guide record once and leaves three compact
//           float4 planes: N with the valid flag in .w, P, and the colour C
//           (demodulated where the albedo allows);
//   pass    one launch per pass j, stride s = 2^j, ping-ponging two colour
//           planes.  The cells with equal (x mod s, y mod s) form a decimated
//           image on which the 25 taps are a dense 5x5: a 256-thread workgroup
//           takes a 16x16 tile of one residue class, stages its 20x20 halo of
//           N, P and C in LDS (19.2 KB) with loads of stride s, and every lane
//           runs its taps from there, in the order of the definition;
//   final   remodulates and writes the float image and / or the RGBA8 one.
// Every weight is a fixed sequence of fp32 operations (-ffp-contract=off), so
// the result equals tests/denoise_driver.c bit for bit.
//
// LDS reads.  ds_read_b128 serves a wave in four groups of 16 lanes, {0-3,
// 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, and a group is
// conflict-free when its 16 addresses fall into the 16 distinct 16-byte slots
// of a 256-byte bank row.  With the row-major lane order (lane l at column
// l % 16, row l / 16) a group spans two tile rows and a pitch of 20 cells
// would put columns 12-15 of one row and 8-11 of the next on the same slots.
// Instead of padding the rows to 32 cells (30 KB), the lanes are dealt so that
// each group IS one row of 16 consecutive cells: column l % 16, row
// 2 * (l / 32) + (((l / 16) & 1) ^ (column in 4..11)).  Sixteen consecutive
// 16-byte cells cover every slot once at any pitch and any tap offset, so the
// 20-cell pitch stays and no read conflicts.
//
// Measured against it and not shipped (profiles/denoise/README.md): a kernel
// with no LDS tile, one lane per cell in row-major order, the 25 taps gathered
// from the planes in global memory through L2.  It takes 1.4 times as long per
// call at five passes; from stride 16 on it is the faster of the two.
#include <hip/hip_runtime.h>

#include "vr_denoise.hpp"
#include "vr_kernel.hpp"

namespace vr {

namespace {

constexpr int kTile = 16, kHalo = kTile + 4;
constexpr float kAlbedoMin = 0x1p-8f;            // demodulate a channel whose albedo is above this

struct PassParams {
    const vr4* N; const vr4* P; const vr4* Cin; vr4* Cout;
    uint32_t w, h, stride, sx, sy, tiles_x, tiles_y, m;
    float kp, kc;
};

// 1.f / x, bit for bit: rcp_rn inside the range its exhaustive test covers
// when every active lane of the wave is there, else the IEEE division
__device__ __forceinline__ float recip_exact(float x)
{
    if (__builtin_expect(__ballot(!(x >= 0x1p-32f && x <= kRcpRnHi)) != 0ull, 0)) return 1.0f / x;
    return rcp_rn(x);
}

// One tap of the definition: the weight of q seen from p, and q's colour added
// to the sums.  h: the B3-spline factor K[|dy|] * K[|dx|].
__device__ __forceinline__ void tap(const vr4& Np, const vr4& Pp, const vr4& Cp, const vr4& Nq, const vr4& Pq, const vr4& Cq,
                                    float h, uint32_t m, float kp, float kc, float& sx, float& sy, float& sz, float& ws)
{
    const float dn = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
    float wn = dn > 0.f ? dn : 0.f;
    for (uint32_t i = 0; i < m; ++i) wn = wn * wn;
    const float ex = Pq.x - Pp.x, ey = Pq.y - Pp.y, ez = Pq.z - Pp.z;
    const float dp = (Np.x * ex + Np.y * ey) + Np.z * ez;
    const float wp = recip_exact(1.f + (dp * dp) * kp);
    const float cx = Cq.x - Cp.x, cy = Cq.y - Cp.y, cz = Cq.z - Cp.z;
    const float d2 = (cx * cx + cy * cy) + cz * cz;
    const float wc = recip_exact(1.f + d2 * kc);
    const float w = ((h * wn) * wp) * wc;
    sx = sx + w * Cq.x;
    sy = sy + w * Cq.y;
    sz = sz + w * Cq.z;
    ws = ws + w;
}

__device__ __forceinline__ vr4 filtered(const vr4& Cp, float sx, float sy, float sz, float ws)
{
    if (!(ws > 0.f)) return Cp;
    const float inv = recip_exact(ws);
    return mk4(sx * inv, sy * inv, sz * inv, Cp.w);
}

__device__ __forceinline__ float spline(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

__global__ void __launch_bounds__(kBlockThreads)
denoise_prep_kernel(const vr4* __restrict__ color, const vr4* __restrict__ accum, float coef, const vr4* __restrict__ rows,
                    uint32_t n, uint32_t demodulate, uint32_t with_guides, vr4* __restrict__ N, vr4* __restrict__ P,
                    vr4* __restrict__ C)
{
    const uint32_t i = blockIdx.x * (uint32_t)kBlockThreads + threadIdx.x;
    if (i >= n) return;
    vr4 c = color ? color[i] : mul4s(accum[i], coef);
    if (with_guides) {
        const vr4* r = rows + 7u * (size_t)i;
        const vr4 head = r[0], pos = r[1], nrm = r[2], alb = r[4];
        const uint32_t kind = __float_as_uint(head.y);
        const bool valid = kind >= 1u && kind <= 4u;
        if (valid && demodulate) {
            if (alb.x > kAlbedoMin) c.x = c.x * recip_exact(alb.x);
            if (alb.y > kAlbedoMin) c.y = c.y * recip_exact(alb.y);
            if (alb.z > kAlbedoMin) c.z = c.z * recip_exact(alb.z);
        }
        N[i] = mk4(nrm.x, nrm.y, nrm.z, valid ? 1.f : 0.f);
        P[i] = pos;
    }
    C[i] = c;
}

__global__ void __launch_bounds__(kBlockThreads) denoise_pass_kernel(const PassParams q)
{
    __shared__ vr4 tN[kHalo * kHalo], tP[kHalo * kHalo], tC[kHalo * kHalo];
    // the residue class and the tile of its decimated image
    const uint32_t gx = q.tiles_x * q.sx, bx = blockIdx.x % gx, by = blockIdx.x / gx;
    const uint32_t rx = bx / q.tiles_x, tx0 = (bx % q.tiles_x) * (uint32_t)kTile;
    const uint32_t ry = by / q.tiles_y, ty0 = (by % q.tiles_y) * (uint32_t)kTile;
    const long long s = (long long)q.stride;
    // the tile's first cell lies outside the grid: nothing to do (the whole block leaves)
    if ((long long)rx + (long long)tx0 * s >= (long long)q.w || (long long)ry + (long long)ty0 * s >= (long long)q.h) return;
    for (int k = (int)threadIdx.x; k < kHalo * kHalo; k += kBlockThreads) {
        const int hx = k % kHalo, hy = k / kHalo;
        const long long x = (long long)rx + ((long long)tx0 + hx - 2) * s;
        const long long y = (long long)ry + ((long long)ty0 + hy - 2) * s;
        vr4 n = mk4(0.f, 0.f, 0.f, 0.f), p = n, c = n;       // outside the grid: invalid
        if (x >= 0 && x < (long long)q.w && y >= 0 && y < (long long)q.h) {
            const size_t i = (size_t)y * q.w + (size_t)x;
            n = q.N[i]; c = q.Cin[i];
            if (n.w != 0.f) p = q.P[i];
        }
        tN[k] = n; tP[k] = p; tC[k] = c;
    }
    __syncthreads();
    // one 16-lane read group per tile row (see the head of the file)
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int lx = lane & 15;
    const int ly = 4 * wave + 2 * (lane >> 5) + (((lane >> 4) & 1) ^ (((lx + 4) >> 3) & 1));
    const long long x = (long long)rx + ((long long)tx0 + lx) * s, y = (long long)ry + ((long long)ty0 + ly) * s;
    if (x >= (long long)q.w || y >= (long long)q.h) return;
    const int kc0 = (ly + 2) * kHalo + lx + 2;
    const vr4 Np = tN[kc0], Cp = tC[kc0];
    const size_t i = (size_t)y * q.w + (size_t)x;
    if (Np.w == 0.f) { q.Cout[i] = Cp; return; }             // an invalid cell keeps its colour
    const vr4 Pp = tP[kc0];
    float sx = 0.f, sy = 0.f, sz = 0.f, ws = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int k = kc0 + dy * kHalo + dx;
            const vr4 Nq = tN[k];
            if (Nq.w == 0.f) continue;
            tap(Np, Pp, Cp, Nq, tP[k], tC[k], spline(dy) * spline(dx), q.m, q.kp, q.kc, sx, sy, sz, ws);
        }
    }
    q.Cout[i] = filtered(Cp, sx, sy, sz, ws);
}

__global__ void __launch_bounds__(kBlockThreads)
denoise_final_kernel(const vr4* __restrict__ C, const vr4* __restrict__ N, const vr4* __restrict__ rows, uint32_t n,
                     uint32_t remodulate, vr4* __restrict__ out, u8x4* __restrict__ out_rgba8, const float* __restrict__ tone_t)
{
    __shared__ float T[256];
    if (out_rgba8) {                    // uniform: the table in LDS, as the render's finish pass keeps it
        T[threadIdx.x] = tone_t[threadIdx.x];
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * (uint32_t)kBlockThreads + threadIdx.x;
    if (i >= n) return;
    vr4 c = C[i];
    if (remodulate && N[i].w != 0.f) {
        const vr4 alb = rows[7u * (size_t)i + 4u];
        if (alb.x > kAlbedoMin) c.x = c.x * alb.x;
        if (alb.y > kAlbedoMin) c.y = c.y * alb.y;
        if (alb.z > kAlbedoMin) c.z = c.z * alb.z;
    }
    if (out) out[i] = c;
    if (out_rgba8) {
        u8x4 b;
        b.x = tone_byte(clampf(c.x, 0.f, 1.f), T);
        b.y = tone_byte(clampf(c.y, 0.f, 1.f), T);
        b.z = tone_byte(clampf(c.z, 0.f, 1.f), T);
        b.w = 0xff;
        out_rgba8[i] = b;
    }
}

} // namespace

static_assert(kBlockThreads == kTile * kTile && kBlockThreads == 256, "one lane per cell of a tile; the tone table is 256 floats");

int launch_denoise(const Denoise& d, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = d.w * d.h;
    const uint32_t blocks = (n + (uint32_t)kBlockThreads - 1u) / (uint32_t)kBlockThreads;
    vr4* N = d.planes; vr4* P = N + n; vr4* C0 = P + n; vr4* C1 = C0 + n;
    const uint32_t passes = d.n_passes;
    const uint32_t demod = passes > 0u && d.demodulate ? 1u : 0u;
    denoise_prep_kernel<<<blocks, kBlockThreads, 0, s>>>(d.color, d.accum, d.coef, (const vr4*)d.guides, n, demod,
                                                         passes > 0u ? 1u : 0u, N, P, C0);
    const float kp = 1.f / (d.sigma_position * d.sigma_position);
    const float kc0 = 1.f / (d.sigma_color * d.sigma_color);
    vr4* in = C0; vr4* outp = C1;
    for (uint32_t j = 0; j < passes; ++j) {
        PassParams q{};
        q.N = N; q.P = P; q.Cin = in; q.Cout = outp;
        q.w = d.w; q.h = d.h; q.stride = 1u << j; q.m = d.normal_pow_log2;
        q.kp = kp; q.kc = kc0 * (float)(1u << (2u * j));
        q.sx = q.stride < d.w ? q.stride : d.w;
        q.sy = q.stride < d.h ? q.stride : d.h;
        const uint32_t dec_w = (d.w + q.stride - 1u) / q.stride, dec_h = (d.h + q.stride - 1u) / q.stride;
        q.tiles_x = (dec_w + (uint32_t)kTile - 1u) / (uint32_t)kTile;
        q.tiles_y = (dec_h + (uint32_t)kTile - 1u) / (uint32_t)kTile;
        // a one-dimensional grid: a 1 x h sheet has more tile rows than a grid's y extent holds
        const uint64_t tiles = (uint64_t)(q.tiles_x * q.sx) * (uint64_t)(q.tiles_y * q.sy);
        if (tiles > 0x7fffffffull) return (int)hipErrorInvalidConfiguration;
        denoise_pass_kernel<<<(uint32_t)tiles, kBlockThreads, 0, s>>>(q);
        vr4* t = in; in = outp; outp = t;
    }
    denoise_final_kernel<<<blocks, kBlockThreads, 0, s>>>(in, N, (const vr4*)d.guides, n, demod, d.out, d.out_rgba8, d.tone_t);
    return (int)hipGetLastError();
}

} // namespace vr
