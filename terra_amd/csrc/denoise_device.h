// denoise_device.h -- what the a-trous filter (denoise_kernels.hip), the moments (variance_kernels.hip) and the temporal reprojection (temporal_kernels.hip)
// share, each defined once: the filter's constants and per-tap weights, the per-pixel inputs, the lane-to-pixel mapping and the variance of a moments entry
// (include/terra_amd.h "Denoiser", "Variance-guided denoiser").
#pragma once
#include <hip/hip_runtime.h>
#include "trace_math.h"

// Constants of the filter (include/terra_amd.h, tests/test_denoise.py restates them)
#define TERRA_DN_SIGMA_C2 0.25f         // sigma_c^2 (sigma_c = 0.5: DESIGN.md "AOV buffers and the denoiser", measured against 1)
#define TERRA_DN_SIGMA_Z  0.05f
#define TERRA_DN_ALBEDO_MIN 0.01f
#define TERRA_DN_NORMAL_MIN 1e-6f
#define TERRA_DN_EPS_C 1e-8f
#define TERRA_DN_EPS_Z 1e-6f
// guide state (g1.w): 0 no samples, 1 valid, 2 samples but a non-finite mean (filled from its neighbours in iteration 0)

TD float dn_max ( float a, float b ) { return a > b ? a : b; }
TD bool dn_finite ( float v ) { return ( __float_as_uint ( v ) & 0x7f800000u ) != 0x7f800000u; }
TD float dn_lum ( float x, float y, float z ) { return 0.2126f * x + 0.7152f * y + 0.0722f * z; }
// The "Denoiser" section's per-pixel quantities of frame pixel `pix`: res (the result word), samples, n = float(samples), c = acc / samples, finite (VALID:
// samples > 0 and c finite), a0 / a1 (the AOV entry's first two words), a / z / nv (the means over the hits, all zero without one; nv normalised, zero if its
// length <= 1e-6). Shared by the a-trous prepass (denoise_kernels.hip) and the temporal reprojection (temporal_kernels.hip).
struct DnPixel { float4 res; int samples; float n; V3 c; bool finite; float4 a0, a1; V3 a, nv; float z; };
TD DnPixel dn_pixel ( const float4* results, const float4* aov, size_t pix ) {
    DnPixel p;
    p.res = results[pix];
    p.samples = __float_as_int ( p.res.w );
    p.n = ( float ) p.samples;
    p.c = v3 ( p.res.x / p.n, p.res.y / p.n, p.res.z / p.n );
    p.finite = p.samples > 0 && dn_finite ( p.c.x ) && dn_finite ( p.c.y ) && dn_finite ( p.c.z );
    p.a0 = aov[3 * pix]; p.a1 = aov[3 * pix + 1];
    p.a = v3 ( 0.f, 0.f, 0.f ); p.nv = v3 ( 0.f, 0.f, 0.f );
    p.z = 0.f;
    if ( p.a0.w > 0.f ) {
        p.a = v3 ( p.a0.x / p.a0.w, p.a0.y / p.a0.w, p.a0.z / p.a0.w );
        p.z = p.a1.w / p.a0.w;
        p.nv = v3 ( p.a1.x / p.a0.w, p.a1.y / p.a0.w, p.a1.z / p.a0.w );
        const float len = length ( p.nv );
        p.nv = len > TERRA_DN_NORMAL_MIN ? v3 ( p.nv.x / len, p.nv.y / len, p.nv.z / len ) : v3 ( 0.f, 0.f, 0.f );
    }
    return p;
}
// The lane's pixel under 16 x 16 blocks laid over a w x h rectangle at (x, y) of a frame fb_w pixels wide: (lx, ly) in the rectangle, pix its index in the frame,
// i its index in the rectangle (the filter's planes). !inside: the lane lies beyond the rectangle's edge and has nothing to do (pix and i are then no pixel's).
// (Returned by value: filled through a reference, the variance-guided step took two more registers and measured 1 % slower.)
struct DnLane { bool inside; uint32_t lx, ly; size_t pix, i; };
TD DnLane dn_lane ( uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h ) {
    DnLane l;
    l.lx = blockIdx.x * 16u + threadIdx.x; l.ly = blockIdx.y * 16u + threadIdx.y;
    l.inside = l.lx < w && l.ly < h;
    l.pix = ( size_t ) ( y + l.ly ) * fb_w + ( x + l.lx ); l.i = ( size_t ) l.ly * w + l.lx;
    return l;
}
// var of the pixel's mean luminance from the second word of its moments entry (mean, m2, batches, weight); negative: unknown
TD float var_of ( const float4& m1 ) {
    const int batches = __float_as_int ( m1.z ), weight = __float_as_int ( m1.w );
    return batches >= 2 ? m1.y / ( ( float ) weight * ( float ) ( batches - 1 ) ) : -1.f;
}
TD V3 dn_demodulate ( V3 c, V3 a ) { return v3 ( c.x / dn_max ( a.x, TERRA_DN_ALBEDO_MIN ), c.y / dn_max ( a.y, TERRA_DN_ALBEDO_MIN ), c.z / dn_max ( a.z, TERRA_DN_ALBEDO_MIN ) ); }      // u = c / max(a, 0.01)
TD float4 dn_valid4 ( V3 u ) { return make_float4 ( u.x, u.y, u.z, 1.f ); }
TD float dn_kernel ( int d ) { const float kh[5] = { 1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f }; return kh[d + 2]; }       // h(d), d in -2 .. 2
// w_c of the a-trous filter: the squared colour distance against the two luminances
TD float dn_weight_colour ( const float4& up, const float4& uq, float lp, float lq, float sigma_c2 ) {
    const float ex = up.x - uq.x, ey = up.y - uq.y, ez = up.z - uq.z;
    return expf ( -( ( ex * ex + ey * ey + ez * ez ) / ( sigma_c2 * ( lp * lp + lq * lq ) + TERRA_DN_EPS_C ) ) );
}
// w_n and w_z from the guide words (normal.xyz, depth) of the two pixels; zs = sigma_z * step
TD float dn_weight_normal ( const float4& gp, const float4& gq, bool np_zero ) {
    const bool nq_zero = gq.x == 0.f && gq.y == 0.f && gq.z == 0.f;
    if ( np_zero || nq_zero ) return ( np_zero && nq_zero ) ? 1.f : 0.f;
    float wn = dn_max ( 0.f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z );
    #pragma unroll
    for ( int k = 0; k < 7; ++k ) wn = wn * wn;          // ^128
    return wn;
}
TD float dn_weight_depth ( const float4& gp, const float4& gq, float zs ) { return expf ( -( fabsf ( gp.w - gq.w ) / ( zs * dn_max ( gp.w, gq.w ) + TERRA_DN_EPS_Z ) ) ); }
