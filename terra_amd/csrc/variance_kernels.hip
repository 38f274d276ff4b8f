// variance_kernels.hip -- per-pixel second moments from batch means, the tile error built on them, and the variance-guided a-trous filter
// (include/terra_amd.h "Moments buffer", "Tile error", "Variance-guided denoiser"; DESIGN.md "Variance: moments, guided denoise, adaptive tiles").
//
// Nothing here touches the render: the framebuffer's running sums are read after a render call, and the change since the last look is one batch.
// No atomics anywhere: the same inputs give the same bits. The build compiles without FMA contraction, so each formula below is the header's, operation by operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include "denoise_device.h"
#include "kernels.h"

struct DevMoments { float seen_acc[3]; int seen_samples; float mean; float m2; int batches; int weight; };         // TerraAmdMoments
static_assert ( sizeof ( DevMoments ) == 32, "DevMoments must be 32 bytes" );

#ifndef TERRA_VAR_SIGMA_L               // (both may be set on the command line for an experiment build: build.py's variant; tools/variance_sweep.py)
#define TERRA_VAR_SIGMA_L 8.0f          // sigma_l (include/terra_amd.h; DESIGN.md records what was tried)
#endif
#define TERRA_VAR_EPS_L 1e-6f
#ifndef TERRA_VAR_PREFILTER_CAP
#define TERRA_VAR_PREFILTER_CAP 4.0f
#endif
#define TERRA_VAR_EPS_E 1e-3f
#define TERRA_VAR_LUM_MIN 1e-6f

// var of the pixel's mean luminance from its second word (mean, m2, batches, weight); negative: unknown
TD float var_of ( const float4& m1 ) {
    const int batches = __float_as_int ( m1.z ), weight = __float_as_int ( m1.w );
    return batches >= 2 ? m1.y / ( ( float ) weight * ( float ) ( batches - 1 ) ) : -1.f;
}

// ---- accumulate: one lane per pixel, the entry read and written as two float4 -------------------------------------------------------------------
__global__ __launch_bounds__ ( 256 ) void terra_moments_accumulate ( const float4* results, float4* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h ) {
    const uint32_t lx = blockIdx.x * 16u + threadIdx.x, ly = blockIdx.y * 16u + threadIdx.y;
    if ( lx >= w || ly >= h ) return;
    const size_t pix = ( size_t ) ( y + ly ) * fb_w + ( x + lx );
    const float4 res = results[pix];
    float4 m0 = moments[2 * pix], m1 = moments[2 * pix + 1];
    const int samples = __float_as_int ( res.w );
    int dn = samples - __float_as_int ( m0.w );
    if ( dn == 0 ) return;
    if ( dn < 0 ) {                     // the framebuffer was cleared: start over
        m0 = make_float4 ( 0.f, 0.f, 0.f, __int_as_float ( 0 ) ); m1 = make_float4 ( 0.f, 0.f, __int_as_float ( 0 ), __int_as_float ( 0 ) );
        dn = samples;
    }
    if ( dn > 0 ) {
        const float fn = ( float ) dn;
        const float l = dn_lum ( ( res.x - m0.x ) / fn, ( res.y - m0.y ) / fn, ( res.z - m0.z ) / fn );
        if ( dn_finite ( l ) ) {
            const int W = __float_as_int ( m1.w ) + dn;
            const float d = l - m1.x;
            const float mean = m1.x + ( d * fn ) / ( float ) W;
            m1.y = m1.y + ( fn * d ) * ( l - mean );
            m1.x = mean;
            m1.z = __int_as_float ( __float_as_int ( m1.z ) + 1 );
            m1.w = __int_as_float ( W );
        }
        m0 = make_float4 ( res.x, res.y, res.z, res.w );
    }
    moments[2 * pix] = m0; moments[2 * pix + 1] = m1;
}

hipError_t terra_launch_moments_accumulate ( const void* results, void* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, hipStream_t stream ) {
    if ( w == 0 || h == 0 ) return hipSuccess;
    hipLaunchKernelGGL ( terra_moments_accumulate, dim3 ( ( w + 15u ) / 16u, ( h + 15u ) / 16u ), dim3 ( 16, 16 ), 0, stream,
                         reinterpret_cast<const float4*> ( results ), reinterpret_cast<float4*> ( moments ), fb_w, x, y, w, h );
    return hipGetLastError();
}

// ---- tile error: one 256-lane block per tile ------------------------------------------------------------------------------------------------------
// Lane t sums pixels t, t + 256, ... of the tile (row-major inside the clipped tile), a wave folds its 64 sums with shuffles (offsets 32 .. 1), lane 0 of the block
// adds the four wave sums in wave order.
TD float wave_fold ( float v ) {
    #pragma unroll
    for ( int off = 32; off >= 1; off >>= 1 ) v = v + __shfl_down ( v, off, 64 );
    return v;
}
__global__ __launch_bounds__ ( 256 ) void terra_tile_error ( const float4* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t tile, uint32_t tiles_x, float* errors ) {
    __shared__ float fold[3][4];
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint32_t x0 = tx * tile, y0 = ty * tile;
    const uint32_t tw = w - x0 < tile ? w - x0 : tile, th = h - y0 < tile ? h - y0 : tile, n = tw * th;
    float sv = 0.f, sm = 0.f, unknown = 0.f;
    for ( uint32_t i = tid; i < n; i += 256u ) {
        const uint32_t py = i / tw, px = i - py * tw;
        const float4 m1 = moments[2 * ( ( size_t ) ( y + y0 + py ) * fb_w + ( x + x0 + px ) ) + 1];
        if ( __float_as_int ( m1.z ) < 2 ) unknown = unknown + 1.f;          // (by the batch count alone: rounding may leave an m2 a hair below zero)
        else { sv = sv + var_of ( m1 ); sm = sm + m1.x; }
    }
    sv = wave_fold ( sv ); sm = wave_fold ( sm ); unknown = wave_fold ( unknown );
    if ( ( tid & 63u ) == 0u ) { fold[0][tid >> 6] = sv; fold[1][tid >> 6] = sm; fold[2][tid >> 6] = unknown; }
    __syncthreads();
    if ( tid == 0 ) {
        const float tv = ( ( fold[0][0] + fold[0][1] ) + fold[0][2] ) + fold[0][3], tm = ( ( fold[1][0] + fold[1][1] ) + fold[1][2] ) + fold[1][3];
        const float tu = ( ( fold[2][0] + fold[2][1] ) + fold[2][2] ) + fold[2][3];
        const float fn = ( float ) n;
        errors[t] = tu > 0.f ? INFINITY : sqrtf ( dn_max ( tv, 0.f ) / fn ) / ( tm / fn + TERRA_VAR_EPS_E );
    }
}

hipError_t terra_launch_tile_error ( const void* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t tile, float* errors, hipStream_t stream ) {
    if ( w == 0 || h == 0 ) return hipSuccess;
    if ( tile == 0 || ( uint64_t ) tile * tile >= ( 1ull << 32 ) ) return hipErrorInvalidValue;
    const uint32_t tiles_x = ( w + tile - 1 ) / tile, tiles_y = ( h + tile - 1 ) / tile;
    hipLaunchKernelGGL ( terra_tile_error, dim3 ( tiles_x * tiles_y ), dim3 ( 256 ), 0, stream, reinterpret_cast<const float4*> ( moments ), fb_w, x, y, w, h, tile, tiles_x, errors );
    return hipGetLastError();
}

// ---- variance-guided denoiser -----------------------------------------------------------------------------------------------------------------------
// The prepass and the finish are the a-trous filter's own kernels (aov_kernels.hip); the steps here carry a plane v beside u: the variance of l(u_p), negative where
// it is unknown. (u.w cannot carry it: it is the validity flag, and 0 is a variance a pixel may well have.)
__global__ __launch_bounds__ ( 256 ) void terra_variance_init ( const float4* results, const float4* moments, const float4* u, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, float* v ) {
    const uint32_t lx = blockIdx.x * 16u + threadIdx.x, ly = blockIdx.y * 16u + threadIdx.y;
    if ( lx >= w || ly >= h ) return;
    const size_t pix = ( size_t ) ( y + ly ) * fb_w + ( x + lx ), i = ( size_t ) ly * w + lx;
    const float4 up = u[i];
    float out = -1.f;
    if ( up.w != 0.f ) {                // valid: samples > 0, a finite mean
        const float var = var_of ( moments[2 * pix + 1] );
        if ( var >= 0.f ) {
            const float4 res = results[pix];
            const float n = ( float ) __float_as_int ( res.w );
            const float r = dn_lum ( up.x, up.y, up.z ) / dn_max ( dn_lum ( res.x / n, res.y / n, res.z / n ), TERRA_VAR_LUM_MIN );
            out = var * ( r * r );
            if ( ! ( out >= 0.f ) || !dn_finite ( out ) ) out = -1.f;
        }
    }
    v[i] = out;
}

// iteration `it` (step 2^it) of the a-trous filter with the colour weight taken from the centre's variance where that is known
__global__ __launch_bounds__ ( 256 ) void terra_variance_step ( const float4* g0, const float4* g1, const float4* uin, const float* vin, float4* uout, float* vout, uint32_t w, uint32_t h, int it ) {
    const uint32_t lx = blockIdx.x * 16u + threadIdx.x, ly = blockIdx.y * 16u + threadIdx.y;
    if ( lx >= w || ly >= h ) return;
    const size_t i = ( size_t ) ly * w + lx;
    const float4 up = uin[i];
    const bool pending = it == 0 && g1[i].w == 2.f;
    if ( up.w == 0.f && !pending ) { uout[i] = make_float4 ( 0.f, 0.f, 0.f, 0.f ); vout[i] = -1.f; return; }
    const float vp = vin[i];
    const bool known = !pending && vp >= 0.f;
    const float4 gp = g0[i];
    const bool np_zero = gp.x == 0.f && gp.y == 0.f && gp.z == 0.f;
    float tol = 0.f;
    if ( known ) {                      // g_p: the 3x3 Gaussian of min(v_q, 4 v_p) over the valid neighbours with known variance, each weighted by w_n w_z (step 1) too, renormalised
        float gs = 0.f, gw = 0.f;       // by the weights present (the centre's is 1/4): variance is pooled from the surface the filter averages over, not from across a geometric edge
        const float cap = TERRA_VAR_PREFILTER_CAP * vp;      // a neighbour counts with at most this much: a firefly next door must not widen a quiet pixel's tolerance
        for ( int dy = -1; dy <= 1; ++dy ) {
            const int qy = ( int ) ly + dy;
            if ( qy < 0 || qy >= ( int ) h ) continue;
            for ( int dx = -1; dx <= 1; ++dx ) {
                const int qx = ( int ) lx + dx;
                if ( qx < 0 || qx >= ( int ) w ) continue;
                const size_t q = ( size_t ) qy * w + qx;
                const float vq = vin[q];
                if ( uin[q].w == 0.f || ! ( vq >= 0.f ) ) continue;
                const float4 gq = g0[q];
                const float k = ( ( ( dx == 0 ? 0.5f : 0.25f ) * ( dy == 0 ? 0.5f : 0.25f ) ) * dn_weight_normal ( gp, gq, np_zero ) ) * dn_weight_depth ( gp, gq, TERRA_DN_SIGMA_Z );
                gs = gs + k * ( vq < cap ? vq : cap ); gw = gw + k;
            }
        }
        tol = TERRA_VAR_SIGMA_L * sqrtf ( gs / gw ) + TERRA_VAR_EPS_L;
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
            if ( known ) {
                const float vq = vin[q];
                if ( vq >= 0.f ) { swk = swk + W; sv = sv + ( W * W ) * vq; }
            }
        }
    }
    uout[i] = sw > 0.f ? make_float4 ( sx / sw, sy / sw, sz / sw, 1.f ) : make_float4 ( 0.f, 0.f, 0.f, 0.f );
    vout[i] = ( known && sw > 0.f && swk > 0.f ) ? sv / ( swk * swk ) : -1.f;
}

hipError_t terra_launch_denoise_variance ( const void* results, const void* aov, const void* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, int iterations,
                                           float exposure, int op, float gamma, float* radiance, float* pixels, hipStream_t stream ) {
    if ( w == 0 || h == 0 || ( !radiance && !pixels ) ) return hipSuccess;
    const dim3 grid ( ( w + 15u ) / 16u, ( h + 15u ) / 16u ), block ( 16, 16 );
    const size_t n = ( size_t ) w * h;
    float4* scratch = nullptr;
    if ( iterations > 0 ) { const hipError_t e = hipMallocAsync ( ( void** ) &scratch, 4 * n * sizeof ( float4 ) + 2 * n * sizeof ( float ), stream ); if ( e != hipSuccess ) return e; }
    float4* g0 = scratch; float4* g1 = scratch ? scratch + n : nullptr; float4* ua = scratch ? scratch + 2 * n : nullptr; float4* ub = scratch ? scratch + 3 * n : nullptr;
    float* va = scratch ? reinterpret_cast<float*> ( scratch + 4 * n ) : nullptr; float* vb = va ? va + n : nullptr;
    hipError_t e = hipSuccess;
    if ( iterations > 0 ) {
        e = terra_launch_denoise_prepass ( results, aov, fb_w, x, y, w, h, g0, g1, ua, stream );
        if ( e == hipSuccess ) {
            hipLaunchKernelGGL ( terra_variance_init, grid, block, 0, stream, reinterpret_cast<const float4*> ( results ), reinterpret_cast<const float4*> ( moments ), ua, fb_w, x, y, w, h, va );
            for ( int it = 0; it < iterations; ++it ) {
                hipLaunchKernelGGL ( terra_variance_step, grid, block, 0, stream, g0, g1, ua, va, ub, vb, w, h, it );
                float4* t = ua; ua = ub; ub = t;
                float* tv = va; va = vb; vb = tv;
            }
            e = hipGetLastError();
        }
    }
    if ( e == hipSuccess ) e = terra_launch_denoise_finish ( results, g1, ua, fb_w, x, y, w, h, iterations, exposure, op, gamma, radiance, pixels, stream );
    if ( scratch ) ( void ) hipFreeAsync ( scratch, stream );
    return e;
}
