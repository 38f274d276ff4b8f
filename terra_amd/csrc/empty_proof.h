// empty_proof.h -- "no camera ray of this pixel block can hit anything", decided in double precision before the launch.
// One definition for the device (terra_block_class_kernel) and the host (scene_host.cpp exports it as terra_amd_empty_proof, which tests/test_empty_skip.py calls
// without a GPU), so it includes nothing of HIP.
//
// A block's FOOTPRINT is the set of film positions its pixels can sample: the pixels clipped to the call's rectangle, widened by the sub-pixel jitter
// (camera_sample, trace_geometry.h) and by a guard of one whole pixel on every side. Its four side planes pass through the camera position; a fifth plane
// through it has the whole film in front. A triangle is SEPARATED when one of the five planes has all three vertices on its outer side by the margin
//     n . (v - c)  >  TERRA_EMPTY_MARGIN_REL * |v - c|  +  (rounding of the ray origin),
// and is not seen edge-on from the camera (the float test's one weak spot). A block is PROVED EMPTY when every triangle is separated.
// Non-finite inputs and degenerate footprints prove nothing.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TERRA_EP_FN __host__ __device__ inline
#else
#define TERRA_EP_FN static inline
#endif

#define TERRA_EMPTY_U 5.9604644775390625e-8            // 2^-24: unit roundoff of binary32
#define TERRA_EMPTY_MARGIN_REL ( 32.0 * TERRA_EMPTY_U ) // 11 u of vertex perturbation in the float test + 3 u of its direction, doubled
#define TERRA_EMPTY_EDGE_ON ( 64.0 * TERRA_EMPTY_U )    // camera-to-triangle-plane clearance below which the float edge functions may agree by rounding alone
#define TERRA_EMPTY_GUARD_PIXELS 1.0

struct TerraEmptyPlanes {
    double n[5][3];     // unit outward normals, world space; the planes pass through c
    double c[3];        // camera position
    double origin_slack; // absolute part of the margin: the rounding of the kernel's ray origin fl(c + fl(0.001 d))
    int ok;             // 0: nothing can be proved with these planes
};

TERRA_EP_FN int terra_ep_finite ( double x ) { return x - x == 0.0; }

// [x0, x1) x [y0, y1): the block's pixels in frame coordinates, already clipped to the rectangle
TERRA_EP_FN TerraEmptyPlanes terra_empty_planes ( const float* cam_rot, const float* cam_pos, float tan_half_fov, float aspect, float jitter,
                                                   uint32_t fb_w, uint32_t fb_h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1 ) {
    TerraEmptyPlanes P;
    P.ok = 0; P.origin_slack = 0.0;
    for ( int k = 0; k < 5; ++k ) for ( int a = 0; a < 3; ++a ) P.n[k][a] = 0.0;
    for ( int a = 0; a < 3; ++a ) P.c[a] = ( double ) cam_pos[a];
    double R[9];
    int fin = terra_ep_finite ( ( double ) tan_half_fov ) && terra_ep_finite ( ( double ) aspect ) && terra_ep_finite ( ( double ) jitter );
    for ( int i = 0; i < 9; ++i ) { R[i] = ( double ) cam_rot[i]; fin = fin && terra_ep_finite ( R[i] ); }
    for ( int a = 0; a < 3; ++a ) fin = fin && terra_ep_finite ( P.c[a] );
    if ( !fin || fb_w == 0 || fb_h == 0 || x1 <= x0 || y1 <= y0 ) return P;
    const double j = fabs ( ( double ) jitter ) + TERRA_EMPTY_GUARD_PIXELS;
    // film positions as camera_sample makes them: ndc = (pixel + 0.5 + d) / size, s = 2 ndc - 1 (x), 1 - 2 ndc (y), f = s * (aspect) * tan_half_fov
    const double sx_a = 2.0 * ( ( double ) x0 + 0.5 - j ) / ( double ) fb_w - 1.0, sx_b = 2.0 * ( ( double ) ( x1 - 1u ) + 0.5 + j ) / ( double ) fb_w - 1.0;
    const double sy_a = 1.0 - 2.0 * ( ( double ) y0 + 0.5 - j ) / ( double ) fb_h, sy_b = 1.0 - 2.0 * ( ( double ) ( y1 - 1u ) + 0.5 + j ) / ( double ) fb_h;
    const double kx = ( double ) aspect * ( double ) tan_half_fov, ky = ( double ) tan_half_fov;
    double fx_lo = sx_a * kx, fx_hi = sx_b * kx, fy_lo = sy_a * ky, fy_hi = sy_b * ky;
    if ( fx_lo > fx_hi ) { const double t = fx_lo; fx_lo = fx_hi; fx_hi = t; }
    if ( fy_lo > fy_hi ) { const double t = fy_lo; fy_lo = fy_hi; fy_hi = t; }
    if ( ! ( fx_hi > fx_lo && fy_hi > fy_lo ) || !terra_ep_finite ( fx_hi - fx_lo ) || !terra_ep_finite ( fy_hi - fy_lo ) ) return P;      // degenerate footprint (a zero field of view)
    // world direction of the camera-space vector (fx, fy, fz): the rotation camera_sample applies
    #define TERRA_EP_DIR( out, fx, fy, fz ) { out[0] = R[0] * ( fx ) + R[1] * ( fy ) + R[2] * ( fz ); out[1] = R[3] * ( fx ) + R[4] * ( fy ) + R[5] * ( fz ); out[2] = R[6] * ( fx ) + R[7] * ( fy ) + R[8] * ( fz ); }
    double corner[4][3], centre[3], ex[3], ey[3];
    TERRA_EP_DIR ( corner[0], fx_lo, fy_lo, 1.0 ); TERRA_EP_DIR ( corner[1], fx_hi, fy_lo, 1.0 );
    TERRA_EP_DIR ( corner[2], fx_hi, fy_hi, 1.0 ); TERRA_EP_DIR ( corner[3], fx_lo, fy_hi, 1.0 );
    TERRA_EP_DIR ( centre, 0.5 * ( fx_lo + fx_hi ), 0.5 * ( fy_lo + fy_hi ), 1.0 );
    TERRA_EP_DIR ( ex, 1.0, 0.0, 0.0 ); TERRA_EP_DIR ( ey, 0.0, 1.0, 0.0 );
    #undef TERRA_EP_DIR
    // plane k = 0 .. 3 is spanned by two neighbouring corner directions (whatever cam_rot is, orthonormal or not); plane 4 by the film's two axes
    for ( int k = 0; k < 5; ++k ) {
        const double* a = k < 4 ? corner[k] : ex; const double* b = k < 4 ? corner[( k + 1 ) & 3] : ey;
        double n[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
        const double len = sqrt ( n[0] * n[0] + n[1] * n[1] + n[2] * n[2] );
        if ( ! ( len > 0.0 ) || !terra_ep_finite ( len ) ) return P;
        double side = ( n[0] * centre[0] + n[1] * centre[1] + n[2] * centre[2] ) / len;      // the footprint's centre must lie strictly inside
        const double clen = sqrt ( centre[0] * centre[0] + centre[1] * centre[1] + centre[2] * centre[2] );
        if ( ! ( fabs ( side ) > TERRA_EMPTY_MARGIN_REL * clen ) ) return P;
        const double s = side > 0.0 ? -1.0 / len : 1.0 / len;                               // outward: away from the centre
        for ( int q = 0; q < 3; ++q ) P.n[k][q] = n[q] * s;
    }
    P.origin_slack = 4.0 * TERRA_EMPTY_U * ( fabs ( P.c[0] ) + fabs ( P.c[1] ) + fabs ( P.c[2] ) + 1e-3 );
    P.ok = 1;
    return P;
}

// 1: no ray from the camera through the footprint can meet triangle (a, b, c), and the render kernel's float test says so too
TERRA_EP_FN int terra_empty_separates ( const TerraEmptyPlanes& P, const float* a, const float* b, const float* c ) {
    if ( !P.ok ) return 0;
    double v[3][3], d[3];
    for ( int q = 0; q < 3; ++q ) { v[0][q] = ( double ) a[q] - P.c[q]; v[1][q] = ( double ) b[q] - P.c[q]; v[2][q] = ( double ) c[q] - P.c[q]; }
    double dmax = 0.0;
    for ( int i = 0; i < 3; ++i ) {
        d[i] = sqrt ( v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] );
        if ( !terra_ep_finite ( d[i] ) ) return 0;
        if ( d[i] > dmax ) dmax = d[i];
    }
    // edge-on: six times the volume of the tetrahedron (camera, a, b, c) against (largest distance)^2 x (longest edge); also refuses zero-area triangles
    {
        const double e1[3] = { v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2] }, e2[3] = { v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2] }, e3[3] = { v[2][0] - v[1][0], v[2][1] - v[1][1], v[2][2] - v[1][2] };
        const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        const double vol6 = fabs ( nx * v[0][0] + ny * v[0][1] + nz * v[0][2] );
        double l2 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2];
        const double l2b = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2], l2c = e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2];
        if ( l2b > l2 ) l2 = l2b;
        if ( l2c > l2 ) l2 = l2c;
        if ( ! ( vol6 > TERRA_EMPTY_EDGE_ON * dmax * dmax * sqrt ( l2 ) ) ) return 0;
    }
    for ( int k = 0; k < 5; ++k ) {
        int out = 1;
        for ( int i = 0; i < 3; ++i ) {
            const double s = P.n[k][0] * v[i][0] + P.n[k][1] * v[i][1] + P.n[k][2] * v[i][2];
            out = out && ( s > TERRA_EMPTY_MARGIN_REL * d[i] + P.origin_slack );
        }
        if ( out ) return 1;
    }
    return 0;
}
