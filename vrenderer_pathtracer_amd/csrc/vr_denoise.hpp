// vr_denoise.hpp -- the edge-avoiding a-trous filter (vrhip_denoise,
// vrhip_denoise_frame): the launchers, plain C++ for the host half.  No
// reference counterpart: the reference shows its accumulation unfiltered.
// The filter is defined pixel by pixel in include/vrhip.h (B3-spline taps at
// stride 2^j, weighted by the guides' normals, the plane distance of their
// positions and the colour difference, every weight rational: no
// transcendental function, so that a C restatement, tests/denoise_driver.c,
// gives the kernels' bits).  Kernels: vr_denoise.hip.
#pragma once
#include <stdint.h>

#include "vr_params.hpp"
#include "vr_surface.hpp"

namespace vr {

constexpr uint32_t kDenoiseMaxPasses = 8u;       // stride 128 at the most
constexpr uint32_t kDenoiseMaxNormalPow = 8u;    // wn = max(dn, 0)^(2^m), m <= 8
constexpr uint32_t kDenoisePlanes = 4u;          // float4 planes of scratch per cell: N, P and two colours

// One call of the filter; every pointer is a device pointer, 16-byte aligned.
struct Denoise {
    const vr4* color;            // [w h] the radiance; nullptr: accum * coef (the frame call)
    const vr4* accum; float coef;
    const SurfaceHit* guides;    // [w h]; unread when n_passes == 0
    uint32_t w, h;               // w h < 2^31
    uint32_t n_passes;           // <= kDenoiseMaxPasses
    uint32_t demodulate;         // 0 or 1
    uint32_t normal_pow_log2;    // <= kDenoiseMaxNormalPow
    float sigma_color, sigma_position;   // finite, > 0
    vr4* planes;                 // kDenoisePlanes * w h float4 of scratch
    vr4* out;                    // [w h] or nullptr; may be `color`
    u8x4* out_rgba8;             // [w h] or nullptr: tone_byte(clampf(c, 0, 1)) per channel, alpha 0xff
    const float* tone_t;         // the tonemap threshold table; read with out_rgba8 only
};

// Enqueues prep, n_passes passes and the final kernel on `stream`; 0 or a
// hipError_t.  At least one of out and out_rgba8 is set.
int launch_denoise(const Denoise& q, void* stream);

} // namespace vr
