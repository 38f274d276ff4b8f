// temporal_kernels.hip -- temporal reprojection of a per-pixel history across camera moves (include/terra_amd.h "Temporal reprojection"; DESIGN.md
// "Temporal reprojection").
//
// Nothing here touches the render: the framebuffer and the AOV buffer are read after a frame's render and AOV call, last frame's history is read at the place the
// pixel's surface had under the previous camera, and the blended history is written to a second buffer. One lane per pixel; every history, AOV and result access is
// written in the source as a 16-byte float4 load or store (three per history tap; where only one or two components of a word are used, the compiler narrows that load
// to 4 or 8 bytes in the gfx950 code, which moves no more memory); no LDS (the taps of neighbouring lanes meet in the caches), no atomics: the same inputs give the
// same bits. The build compiles without FMA contraction, so each formula below is the header's, operation by operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include "trace_geometry.h"
#include "denoise_device.h"
#include "kernels.h"

struct DevHistory { float radiance[3]; float length; float normal[3]; float depth; float mu1, mu2; float reserved[2]; };        // TerraAmdHistory
static_assert ( sizeof ( DevHistory ) == 48, "DevHistory must be 48 bytes" );

#define TERRA_TMP_SNAP ( 1.f / 64.f )
#define TERRA_TMP_MIN_WEIGHT 1e-3f
#define TERRA_TMP_LUM_MIN 1e-6f
#define TERRA_TMP_BLOCK_X 32u
#define TERRA_TMP_BLOCK_Y 8u

// what the taps add up to: sums over the accepted taps in tap order, the smallest length among them
struct TapSum { float w, x, y, z, m1, m2, len; };

// Is tap (qx, qy) accepted? (inside the rectangle, not empty, depth and normal agree); loads its three words on the way
TD bool tap_load ( const DevTemporalParams& p, const float4* hin, int qx, int qy, float d, V3 n, bool n_zero, float4& h0, float4& h2 ) {
    if ( qx < ( int ) p.x || qy < ( int ) p.y || qx >= ( int ) ( p.x + p.w ) || qy >= ( int ) ( p.y + p.h ) ) return false;
    const size_t q = ( size_t ) qy * p.fb_w + ( size_t ) qx;
    h0 = hin[3 * q];
    if ( ! ( h0.w > 0.f ) ) return false;
    const float4 h1 = hin[3 * q + 1];
    if ( ! ( fabsf ( d - h1.w ) <= p.depth_tolerance * dn_max ( d, h1.w ) ) ) return false;
    const bool q_zero = h1.x == 0.f && h1.y == 0.f && h1.z == 0.f;
    if ( n_zero || q_zero ) { if ( ! ( n_zero && q_zero ) ) return false; }
    else if ( ! ( n.x * h1.x + n.y * h1.y + n.z * h1.z >= p.normal_cos ) ) return false;
    h2 = hin[3 * q + 2];
    return true;
}
TD void tap_add ( const DevTemporalParams& p, const float4* hin, int qx, int qy, float wq, float d, V3 n, bool n_zero, TapSum& s ) {
    float4 h0, h2;
    if ( ! ( wq > 0.f ) || !tap_load ( p, hin, qx, qy, d, n, n_zero, h0, h2 ) ) return;
    s.w = s.w + wq;
    s.x = s.x + wq * h0.x; s.y = s.y + wq * h0.y; s.z = s.z + wq * h0.z;
    s.m1 = s.m1 + wq * h2.x; s.m2 = s.m2 + wq * h2.y;
    s.len = h0.w < s.len ? h0.w : s.len;
}

__global__ __launch_bounds__ ( 256 ) void terra_temporal_reproject ( DevTemporalParams p, const float4* results, const float4* aov, const float4* hin, float4* hout,
                                                                     float4* out_results, float4* out_moments ) {
    const uint32_t lx = blockIdx.x * TERRA_TMP_BLOCK_X + threadIdx.x, ly = blockIdx.y * TERRA_TMP_BLOCK_Y + threadIdx.y;
    if ( lx >= p.w || ly >= p.h ) return;
    const uint32_t px = p.x + lx, py = p.y + ly;
    const size_t pix = ( size_t ) py * p.fb_w + px;
    const DnPixel in = dn_pixel ( results, aov, pix );          // res, samples, n, c, finite, a0, a1, a, nv, z: the "Denoiser" section's, from denoise_device.h
    const V3 A = v3 ( dn_max ( in.a.x, TERRA_DN_ALBEDO_MIN ), dn_max ( in.a.y, TERRA_DN_ALBEDO_MIN ), dn_max ( in.a.z, TERRA_DN_ALBEDO_MIN ) );
    const V3 uc = in.finite ? dn_demodulate ( in.c, in.a ) : v3 ( 0.f, 0.f, 0.f );
    const float lc = dn_lum ( uc.x, uc.y, uc.z );
    const bool n_zero = in.nv.x == 0.f && in.nv.y == 0.f && in.nv.z == 0.f;

    // ---- the history at the place this pixel's surface had under the previous camera ------------------------------------------------------------------
    bool have = false;
    V3 uh = v3 ( 0.f, 0.f, 0.f );
    float m1h = 0.f, m2h = 0.f, nh = 0.f;
    if ( hin && in.a0.w > 0.f ) {
        DevRenderParams rp;                 // the render's own camera function (trace_geometry.h) at the pixel centre: only these fields are read
        rp.jitter = 0.f; rp.fb_w = p.fb_w; rp.fb_h = p.fb_h; rp.inv_fb_w = p.inv_fb_w; rp.inv_fb_h = p.inv_fb_h; rp.aspect = p.aspect; rp.tan_half_fov = p.tan_half_fov;
        #pragma unroll
        for ( int k = 0; k < 9; ++k ) rp.cam_rot[k] = p.cam_rot[k];
        const V3 D = camera_sample ( rp, px, py, 0.f, 0.f );
        const V3 P = v3 ( p.cam_pos[0] + D.x * in.z, p.cam_pos[1] + D.y * in.z, p.cam_pos[2] + D.z * in.z );
        const V3 v = v3 ( P.x - p.prev_pos[0], P.y - p.prev_pos[1], P.z - p.prev_pos[2] );
        const float xc = p.prev_rot[0] * v.x + p.prev_rot[3] * v.y + p.prev_rot[6] * v.z;
        const float yc = p.prev_rot[1] * v.x + p.prev_rot[4] * v.y + p.prev_rot[7] * v.z;
        const float zc = p.prev_rot[2] * v.x + p.prev_rot[5] * v.y + p.prev_rot[8] * v.z;
        if ( zc > 0.f ) {
            const float fx = ( ( ( xc / zc ) / ( p.aspect * p.prev_tan_half_fov ) + 1.f ) / 2.f ) * ( float ) p.fb_w - 0.5f;
            const float fy = ( ( 1.f - ( yc / zc ) / p.prev_tan_half_fov ) / 2.f ) * ( float ) p.fb_h - 0.5f;
            if ( fx >= -1.f && fx < ( float ) p.fb_w && fy >= -1.f && fy < ( float ) p.fb_h ) {        // (a NaN fails; the conversions to int below are in range)
                const float d = length ( v );
                const float rx = floorf ( fx + 0.5f ), ry = floorf ( fy + 0.5f );
                if ( fabsf ( fx - rx ) <= TERRA_TMP_SNAP && fabsf ( fy - ry ) <= TERRA_TMP_SNAP ) {
                    float4 h0, h2;
                    if ( tap_load ( p, hin, ( int ) rx, ( int ) ry, d, in.nv, n_zero, h0, h2 ) ) { have = true; uh = v3 ( h0.x, h0.y, h0.z ); nh = h0.w; m1h = h2.x; m2h = h2.y; }
                } else {
                    const float x0 = floorf ( fx ), y0 = floorf ( fy ), tx = fx - x0, ty = fy - y0;
                    const int ix = ( int ) x0, iy = ( int ) y0;
                    TapSum s; s.w = 0.f; s.x = 0.f; s.y = 0.f; s.z = 0.f; s.m1 = 0.f; s.m2 = 0.f; s.len = INFINITY;
                    tap_add ( p, hin, ix, iy, ( 1.f - tx ) * ( 1.f - ty ), d, in.nv, n_zero, s );
                    tap_add ( p, hin, ix + 1, iy, tx * ( 1.f - ty ), d, in.nv, n_zero, s );
                    tap_add ( p, hin, ix, iy + 1, ( 1.f - tx ) * ty, d, in.nv, n_zero, s );
                    tap_add ( p, hin, ix + 1, iy + 1, tx * ty, d, in.nv, n_zero, s );
                    if ( s.w >= TERRA_TMP_MIN_WEIGHT ) { have = true; uh = v3 ( s.x / s.w, s.y / s.w, s.z / s.w ); m1h = s.m1 / s.w; m2h = s.m2 / s.w; nh = s.len; }
                }
            }
        }
    } else if ( hin && p.same_camera ) {    // a pixel that misses the scene keeps its own history while the camera stands still
        const float4 h0 = hin[3 * pix];
        if ( h0.w > 0.f && hin[3 * pix + 1].w == 0.f ) { const float4 h2 = hin[3 * pix + 2]; have = true; uh = v3 ( h0.x, h0.y, h0.z ); nh = h0.w; m1h = h2.x; m2h = h2.y; }
    }

    // ---- blend --------------------------------------------------------------------------------------------------------------------------------------------
    V3 un = v3 ( 0.f, 0.f, 0.f );
    float m1n = 0.f, m2n = 0.f, len = 0.f, ap = 1.f;
    if ( have ) {
        ap = dn_max ( p.alpha, 1.f / ( nh + 1.f ) );
        if ( in.finite ) {
            un = v3 ( uh.x + ap * ( uc.x - uh.x ), uh.y + ap * ( uc.y - uh.y ), uh.z + ap * ( uc.z - uh.z ) );
            m1n = m1h + ap * ( lc - m1h ); m2n = m2h + ap * ( lc * lc - m2h );
            len = nh + 1.f < p.max_length ? nh + 1.f : p.max_length;
        } else { un = uh; m1n = m1h; m2n = m2h; len = nh; }
    } else if ( in.finite ) { un = uc; m1n = lc; m2n = lc * lc; len = 1.f; }
    hout[3 * pix] = make_float4 ( un.x, un.y, un.z, len );
    hout[3 * pix + 1] = make_float4 ( in.nv.x, in.nv.y, in.nv.z, in.z );
    hout[3 * pix + 2] = make_float4 ( m1n, m2n, 0.f, 0.f );

    // ---- the blended frame as a framebuffer and a moments buffer for the denoisers ----------------------------------------------------------------------
    if ( !out_results && !out_moments ) return;
    float4 o = in.res;
    float4 m1 = make_float4 ( 0.f, 0.f, __int_as_float ( 0 ), __int_as_float ( 0 ) );
    if ( len > 0.f ) {
        const V3 cn = v3 ( un.x * A.x, un.y * A.y, un.z * A.z );
        o = make_float4 ( cn.x * in.n, cn.y * in.n, cn.z * in.n, in.res.w );
        const float lu = dn_lum ( un.x, un.y, un.z );
        if ( len >= 2.f && lu > 0.f ) {
            const float r = dn_max ( dn_lum ( cn.x, cn.y, cn.z ), TERRA_TMP_LUM_MIN ) / lu;
            const float var = ( dn_max ( 0.f, m2n - m1n * m1n ) * ap ) * ( r * r );
            if ( dn_finite ( var ) ) m1 = make_float4 ( m1n, var, __int_as_float ( 2 ), __int_as_float ( 1 ) );
        }
    }
    if ( out_results ) out_results[pix] = o;
    if ( out_moments ) { out_moments[2 * pix] = o; out_moments[2 * pix + 1] = m1; }
}

hipError_t terra_launch_temporal_reproject ( const DevTemporalParams& p, const void* results, const void* aov, const void* history_in, void* history_out,
                                             void* out_results, void* out_moments, hipStream_t stream ) {
    if ( p.w == 0 || p.h == 0 ) return hipSuccess;
    const dim3 grid ( ( p.w + TERRA_TMP_BLOCK_X - 1u ) / TERRA_TMP_BLOCK_X, ( p.h + TERRA_TMP_BLOCK_Y - 1u ) / TERRA_TMP_BLOCK_Y ), block ( TERRA_TMP_BLOCK_X, TERRA_TMP_BLOCK_Y );
    hipLaunchKernelGGL ( terra_temporal_reproject, grid, block, 0, stream, p, reinterpret_cast<const float4*> ( results ), reinterpret_cast<const float4*> ( aov ),
                         reinterpret_cast<const float4*> ( history_in ), reinterpret_cast<float4*> ( history_out ), reinterpret_cast<float4*> ( out_results ),
                         reinterpret_cast<float4*> ( out_moments ) );
    return hipGetLastError();
}
