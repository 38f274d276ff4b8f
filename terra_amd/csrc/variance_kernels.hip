// variance_kernels.hip -- per-pixel second moments from batch means and the tile error built on them (include/terra_amd.h "Moments buffer", "Tile error";
// DESIGN.md "Variance: moments, guided denoise, adaptive tiles"). The filter that is guided by them is denoise_kernels.hip.
//
// Nothing here touches the render: the framebuffer's running sums are read after a render call, and the change since the last look is one batch.
// No atomics anywhere: the same inputs give the same bits. The build compiles without FMA contraction, so each formula below is the header's, operation by operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include "denoise_device.h"
#include "kernels.h"

struct DevMoments { float seen_acc[3]; int seen_samples; float mean; float m2; int batches; int weight; };         // TerraAmdMoments
static_assert ( sizeof ( DevMoments ) == 32, "DevMoments must be 32 bytes" );

#define TERRA_VAR_EPS_E 1e-3f

// ---- accumulate: one lane per pixel, the entry read and written as two float4 -------------------------------------------------------------------
__global__ __launch_bounds__ ( 256 ) void terra_moments_accumulate ( const float4* results, float4* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h ) {
    const DnLane l = dn_lane ( fb_w, x, y, w, h );
    if ( !l.inside ) return;
    const size_t pix = l.pix;
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

// ---- mask from tile errors (include/terra_amd.h "Masked rendering") ----------------------------------------------------------------
// One thread per 16x16 block of the w x h rectangle, row-major: the block belongs to tile (16 bx / tile, 16 by / tile), tiles numbered as terra_tile_error numbers
// them, and is active if `all` or its tile's error exceeds the target -- the adaptive driver's own comparison, so +INFINITY is active, a NaN and equality are not.
__global__ __launch_bounds__ ( 256 ) void terra_error_mask ( const float* errors, uint32_t blocks_x, uint32_t blocks_y, uint32_t tile, uint32_t tiles_x, float target, uint32_t all, uint32_t* mask ) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if ( i >= blocks_x * blocks_y ) return;
    const uint32_t by = i / blocks_x, bx = i - by * blocks_x;
    const float e = errors[ ( size_t ) ( ( by * 16u ) / tile ) * tiles_x + ( bx * 16u ) / tile];
    mask[i] = ( all || e > target ) ? 1u : 0u;
}
hipError_t terra_launch_error_mask ( const float* errors, uint32_t w, uint32_t h, uint32_t tile, float target, int all, uint32_t* mask, hipStream_t stream ) {
    if ( w == 0 || h == 0 ) return hipSuccess;
    if ( tile == 0 || !errors || !mask ) return hipErrorInvalidValue;
    const uint32_t blocks_x = ( w + 15u ) / 16u, blocks_y = ( h + 15u ) / 16u, tiles_x = ( w + tile - 1 ) / tile;
    if ( ( uint64_t ) blocks_x * blocks_y >= ( 1ull << 32 ) ) return hipErrorInvalidValue;
    hipLaunchKernelGGL ( terra_error_mask, dim3 ( ( blocks_x * blocks_y + 255u ) / 256u ), dim3 ( 256 ), 0, stream, errors, blocks_x, blocks_y, tile, tiles_x, target, all ? 1u : 0u, mask );
    return hipGetLastError();
}
