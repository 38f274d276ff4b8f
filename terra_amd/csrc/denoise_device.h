// denoise_device.h -- what the a-trous filter (aov_kernels.hip) and its variance-guided form (variance_kernels.hip) share: the filter's constants and its
// per-tap weights, each defined once (include/terra_amd.h "Denoiser", "Variance-guided denoiser").
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
// The "Denoiser" section's per-pixel quantities, declared as locals of the kernel that names them: res (the result word), samples, n = float(samples),
// c = acc / samples, finite (VALID: samples > 0 and c finite), a0 / a1 (the AOV entry's first two words), a / z / nv (the means over the hits, all zero without one; nv
// normalised, zero if its length <= 1e-6). A macro and not a function so that the a-trous prepass, which had this text before the temporal reprojection shared it,
// still compiles to the same instructions (tools/isa_same.sh): through a function, by value or by reference, the compiler schedules the prepass differently.
// MAINTENANCE HAZARD: the macro injects ten names into the caller's scope (res, samples, n, c, finite, a0, a1, a, nv, z) and `len` into an inner block. A kernel that
// uses it must declare none of the ten itself, may rely on any of them (temporal_kernels.hip reads n), and a `len` of its own must come after the macro. Adding a
// name here means checking both users. If the prepass's instructions are ever allowed to change, replace this with a function that returns a struct.
#define DN_PIXEL_INPUTS( results, aov, pix ) \
    const float4 res = ( results )[pix]; \
    const int samples = __float_as_int ( res.w ); \
    const float n = ( float ) samples; \
    const V3 c = v3 ( res.x / n, res.y / n, res.z / n ); \
    const bool finite = samples > 0 && dn_finite ( c.x ) && dn_finite ( c.y ) && dn_finite ( c.z ); \
    const float4 a0 = ( aov )[3 * ( pix )], a1 = ( aov )[3 * ( pix ) + 1]; \
    V3 a = v3 ( 0.f, 0.f, 0.f ), nv = v3 ( 0.f, 0.f, 0.f ); \
    float z = 0.f; \
    if ( a0.w > 0.f ) { \
        a = v3 ( a0.x / a0.w, a0.y / a0.w, a0.z / a0.w ); \
        z = a1.w / a0.w; \
        nv = v3 ( a1.x / a0.w, a1.y / a0.w, a1.z / a0.w ); \
        const float len = length ( nv ); \
        nv = len > TERRA_DN_NORMAL_MIN ? v3 ( nv.x / len, nv.y / len, nv.z / len ) : v3 ( 0.f, 0.f, 0.f ); \
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
