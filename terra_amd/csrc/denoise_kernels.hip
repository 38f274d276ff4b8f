// denoise_kernels.hip -- the edge-avoiding a-trous denoiser and its variance-guided form (include/terra_amd.h "Denoiser", "Variance-guided denoiser"; DESIGN.md
// "AOV buffers and the denoiser", "Variance: moments, guided denoise, adaptive tiles").
//
// A prepass packs the guides, K step kernels ping-pong the demodulated radiance, a final kernel remodulates and tonemaps. One lane per pixel, 16x16 blocks, every
// plane of the filter indexed over the rectangle. The variance-guided form is the same filter with a plane v beside u: the variance of l(u_p), negative where it
// is unknown (u.w cannot carry it: it is the validity flag, and 0 is a variance a pixel may well have); one step kernel, instantiated with and without it.
// No atomics: the same inputs give the same bits. The build compiles without FMA contraction, so each formula below is the header's, operation by operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include "trace_device.h"
#include "denoise_device.h"
#include "kernels.h"

#ifndef TERRA_VAR_SIGMA_L               // (both may be set on the command line for an experiment build: build.py's variant; tools/variance_sweep.py)
#define TERRA_VAR_SIGMA_L 8.0f          // sigma_l (include/terra_amd.h; DESIGN.md records what was tried)
#endif
#define TERRA_VAR_EPS_L 1e-6f
#ifndef TERRA_VAR_PREFILTER_CAP
#define TERRA_VAR_PREFILTER_CAP 4.0f
#endif
#define TERRA_VAR_LUM_MIN 1e-6f

__global__ __launch_bounds__ ( 256 ) void terra_denoise_prepass ( const float4* results, const float4* aov, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                                                  float4* g0, float4* g1, float4* u ) {
    const DnLane l = dn_lane ( fb_w, x, y, w, h );
    if ( !l.inside ) return;
    const DnPixel p = dn_pixel ( results, aov, l.pix );
    g0[l.i] = make_float4 ( p.nv.x, p.nv.y, p.nv.z, p.z );
    g1[l.i] = make_float4 ( p.a.x, p.a.y, p.a.z, p.finite ? 1.f : ( p.samples > 0 ? 2.f : 0.f ) );
    u[l.i] = p.finite ? dn_valid4 ( dn_demodulate ( p.c, p.a ) ) : make_float4 ( 0.f, 0.f, 0.f, 0.f );
}

// the plane v of the variance-guided form from the moments: var of the mean luminance, scaled to the demodulated signal
__global__ __launch_bounds__ ( 256 ) void terra_variance_init ( const float4* results, const float4* moments, const float4* u, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, float* v ) {
    const DnLane l = dn_lane ( fb_w, x, y, w, h );
    if ( !l.inside ) return;
    const float4 up = u[l.i];
    float out = -1.f;
    if ( up.w != 0.f ) {                // valid: samples > 0, a finite mean
        const float var = var_of ( moments[2 * l.pix + 1] );
        if ( var >= 0.f ) {
            const float4 res = results[l.pix];
            const float n = ( float ) __float_as_int ( res.w );
            const float r = dn_lum ( up.x, up.y, up.z ) / dn_max ( dn_lum ( res.x / n, res.y / n, res.z / n ), TERRA_VAR_LUM_MIN );
            out = var * ( r * r );
            if ( ! ( out >= 0.f ) || !dn_finite ( out ) ) out = -1.f;
        }
    }
    v[l.i] = out;
}

// the variance planes of a step: an argument of the variance-guided instance only
template <bool VARIANCE> struct AtrousV {};
template <> struct AtrousV<true> { const float* in; float* out; };
// iteration `it` (step 2^it): u.w = 1 marks a valid pixel of the input / output. VARIANCE: the colour weight is taken from the centre's variance where that is
// known, and v.in / v.out carry the variance along
template <bool VARIANCE>
__global__ __launch_bounds__ ( 256 ) void terra_atrous_step ( const float4* g0, const float4* g1, const float4* uin, float4* uout, uint32_t w, uint32_t h, int it, AtrousV<VARIANCE> v ) {
    const DnLane l = dn_lane ( w, 0u, 0u, w, h );
    if ( !l.inside ) return;
    const uint32_t lx = l.lx, ly = l.ly;
    const size_t i = l.i;
    const float4 up = uin[i];
    const bool pending = it == 0 && g1[i].w == 2.f;
    if ( up.w == 0.f && !pending ) {
        uout[i] = make_float4 ( 0.f, 0.f, 0.f, 0.f );
        if constexpr ( VARIANCE ) v.out[i] = -1.f;
        return;
    }
    const float4 gp = g0[i];
    const bool np_zero = gp.x == 0.f && gp.y == 0.f && gp.z == 0.f;
    bool known = false;                 // the centre's variance is known (never in the plain instance: what hangs on it folds away)
    float tol = 0.f;
    if constexpr ( VARIANCE ) {
        const float vp = v.in[i];
        known = !pending && vp >= 0.f;
        if ( known ) {                  // g_p: the 3x3 Gaussian of min(v_q, 4 v_p) over the valid neighbours with known variance, each weighted by w_n w_z (step 1) too, renormalised
            float gs = 0.f, gw = 0.f;   // by the weights present (the centre's is 1/4): variance is pooled from the surface the filter averages over, not from across a geometric edge
            const float cap = TERRA_VAR_PREFILTER_CAP * vp;      // a neighbour counts with at most this much: a firefly next door must not widen a quiet pixel's tolerance
            for ( int dy = -1; dy <= 1; ++dy ) {
                const int qy = ( int ) ly + dy;
                if ( qy < 0 || qy >= ( int ) h ) continue;
                for ( int dx = -1; dx <= 1; ++dx ) {
                    const int qx = ( int ) lx + dx;
                    if ( qx < 0 || qx >= ( int ) w ) continue;
                    const size_t q = ( size_t ) qy * w + qx;
                    const float vq = v.in[q];
                    if ( uin[q].w == 0.f || ! ( vq >= 0.f ) ) continue;
                    const float4 gq = g0[q];
                    const float k = ( ( ( dx == 0 ? 0.5f : 0.25f ) * ( dy == 0 ? 0.5f : 0.25f ) ) * dn_weight_normal ( gp, gq, np_zero ) ) * dn_weight_depth ( gp, gq, TERRA_DN_SIGMA_Z );
                    gs = gs + k * ( vq < cap ? vq : cap ); gw = gw + k;
                }
            }
            tol = TERRA_VAR_SIGMA_L * sqrtf ( gs / gw ) + TERRA_VAR_EPS_L;
        }
    }
    const int step = 1 << it;
    const float sigma_c2 = TERRA_DN_SIGMA_C2 * ldexpf ( 1.f, -2 * it ), zs = TERRA_DN_SIGMA_Z * ( float ) step;
    const float lp = dn_lum ( up.x, up.y, up.z );
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, swk = 0.f, sv = 0.f;
    for ( int dy = -2; dy <= 2; ++dy ) {
        const int qy = ( int ) ly + step * dy;
        if ( qy < 0 || qy >= ( int ) h ) continue;
        for ( int dx = -2; dx <= 2; ++dx ) {
            const int qx = ( int ) lx + step * dx;
            if ( qx < 0 || qx >= ( int ) w ) continue;
            const size_t q = ( size_t ) qy * w + qx;
            const float4 uq = uin[q];
            if ( uq.w == 0.f ) continue;
            const float4 gq = g0[q];
            const float lq = dn_lum ( uq.x, uq.y, uq.z );
            const float wc = pending ? 1.f : known ? expf ( -( fabsf ( lp - lq ) / tol ) ) : dn_weight_colour ( up, uq, lp, lq, sigma_c2 );
            const float wn = dn_weight_normal ( gp, gq, np_zero ), wz = dn_weight_depth ( gp, gq, zs );
            const float W = ( ( ( dn_kernel ( dx ) * dn_kernel ( dy ) ) * wc ) * wn ) * wz;
            sw = sw + W; sx = sx + W * uq.x; sy = sy + W * uq.y; sz = sz + W * uq.z;
            if constexpr ( VARIANCE ) {
                if ( known ) {
                    const float vq = v.in[q];
                    if ( vq >= 0.f ) { swk = swk + W; sv = sv + ( W * W ) * vq; }
                }
            }
        }
    }
    uout[i] = sw > 0.f ? make_float4 ( sx / sw, sy / sw, sz / sw, 1.f ) : make_float4 ( 0.f, 0.f, 0.f, 0.f );
    if constexpr ( VARIANCE ) v.out[i] = ( known && sw > 0.f && swk > 0.f ) ? sv / ( swk * swk ) : -1.f;
}

// remodulate and tonemap (iterations == 0: the framebuffer's own mean, as terra_resolve_kernel computes it)
__global__ __launch_bounds__ ( 256 ) void terra_denoise_finish ( const float4* results, const float4* g1, const float4* u, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                                                 int iterations, float exposure, int op, float gamma, float* radiance, float* pixels ) {
    const DnLane l = dn_lane ( fb_w, x, y, w, h );
    if ( !l.inside ) return;
    const size_t pix = l.pix;
    V3 rad = v3 ( 0.f, 0.f, 0.f );
    if ( iterations == 0 ) {
        const float4 res = results[pix];
        const int samples = __float_as_int ( res.w );
        const float n = ( float ) samples;
        if ( samples > 0 ) rad = v3 ( res.x / n, res.y / n, res.z / n );
    } else {
        const float4 uq = u[l.i];
        if ( uq.w != 0.f ) {
            const float4 a = g1[l.i];
            rad = v3 ( uq.x * dn_max ( a.x, TERRA_DN_ALBEDO_MIN ), uq.y * dn_max ( a.y, TERRA_DN_ALBEDO_MIN ), uq.z * dn_max ( a.z, TERRA_DN_ALBEDO_MIN ) );
        }
    }
    if ( radiance ) { radiance[3 * pix] = rad.x; radiance[3 * pix + 1] = rad.y; radiance[3 * pix + 2] = rad.z; }
    if ( pixels ) {
        const V3 color = tonemap ( rad * exposure, op, gamma );
        pixels[3 * pix] = color.x; pixels[3 * pix + 1] = color.y; pixels[3 * pix + 2] = color.z;
    }
}

// prepass -> [init] -> K steps -> finish on one stream-ordered scratch block: four planes of n float4 (g0, g1 and the two u), and with moments two planes of n float
// (the two v) behind them. moments == nullptr: the plain filter.
static hipError_t launch_atrous ( const void* results, const void* aov, const void* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, int iterations,
                                  float exposure, int op, float gamma, float* radiance, float* pixels, hipStream_t stream ) {
    if ( w == 0 || h == 0 || ( !radiance && !pixels ) ) return hipSuccess;
    const dim3 grid ( ( w + 15u ) / 16u, ( h + 15u ) / 16u ), block ( 16, 16 );
    const float4* res = reinterpret_cast<const float4*> ( results );
    const size_t n = ( size_t ) w * h;
    float4* scratch = nullptr;
    if ( iterations > 0 ) {
        const hipError_t e = hipMallocAsync ( ( void** ) &scratch, 4 * n * sizeof ( float4 ) + ( moments ? 2 * n * sizeof ( float ) : 0 ), stream );
        if ( e != hipSuccess ) return e;
    }
    float4* g0 = scratch; float4* g1 = scratch ? scratch + n : nullptr; float4* ua = scratch ? scratch + 2 * n : nullptr; float4* ub = scratch ? scratch + 3 * n : nullptr;
    float* va = scratch && moments ? reinterpret_cast<float*> ( scratch + 4 * n ) : nullptr; float* vb = va ? va + n : nullptr;
    if ( iterations > 0 ) {
        hipLaunchKernelGGL ( terra_denoise_prepass, grid, block, 0, stream, res, reinterpret_cast<const float4*> ( aov ), fb_w, x, y, w, h, g0, g1, ua );
        if ( moments ) hipLaunchKernelGGL ( terra_variance_init, grid, block, 0, stream, res, reinterpret_cast<const float4*> ( moments ), ua, fb_w, x, y, w, h, va );
        for ( int it = 0; it < iterations; ++it ) {
            if ( moments ) hipLaunchKernelGGL ( terra_atrous_step<true>, grid, block, 0, stream, g0, g1, ua, ub, w, h, it, AtrousV<true> { va, vb } );
            else hipLaunchKernelGGL ( terra_atrous_step<false>, grid, block, 0, stream, g0, g1, ua, ub, w, h, it, AtrousV<false> {} );
            float4* t = ua; ua = ub; ub = t;
            float* tv = va; va = vb; vb = tv;
        }
    }
    hipLaunchKernelGGL ( terra_denoise_finish, grid, block, 0, stream, res, g1, ua, fb_w, x, y, w, h, iterations, exposure, op, gamma, radiance, pixels );
    const hipError_t e = hipGetLastError();
    if ( scratch ) ( void ) hipFreeAsync ( scratch, stream );
    return e;
}

hipError_t terra_launch_denoise ( const void* results, const void* aov, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, int iterations,
                                  float exposure, int op, float gamma, float* radiance, float* pixels, hipStream_t stream ) {
    return launch_atrous ( results, aov, nullptr, fb_w, x, y, w, h, iterations, exposure, op, gamma, radiance, pixels, stream );
}
hipError_t terra_launch_denoise_variance ( const void* results, const void* aov, const void* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, int iterations,
                                           float exposure, int op, float gamma, float* radiance, float* pixels, hipStream_t stream ) {
    return launch_atrous ( results, aov, moments, fb_w, x, y, w, h, iterations, exposure, op, gamma, radiance, pixels, stream );
}
