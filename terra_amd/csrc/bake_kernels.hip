// bake_kernels.hip -- lightmap baking (include/terra_amd.h "Lightmap baking" is the definition): the UV-atlas rasteriser that makes the point door's
// points, and gutter dilation. Three kernels:
//   terra_atlas_coverage  one wave per triangle: the triangle's atlas box, grown by the margin, walked in 8 x 8 texel tiles, one texel per lane; every candidate
//                         does one 64-bit atomicMin on the texel's key = (distance2 bits) << 32 | triangle (non-negative binary32 orders as an unsigned integer)
//   terra_atlas_resolve   one lane per texel: the winner's weights made again from the key's triangle by the same function, the point and the texel record written
//   terra_dilate_pass     one lane per texel, one launch per pass, ping-pong between the data and a second copy
// Everything of the rule is binary64 (the unit is built with -ffp-contract=off like the others; binary64 division is IEEE).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace {

struct AtlasTri { double ax, ay, bx, by, cx, cy, area2; bool ok; };

// the triangle's atlas coordinates and area2; ok = it can cover something
__device__ AtlasTri atlas_tri ( const DevScene& sc, const DevAtlas& at, const float* uvs, uint32_t t ) {
    float u[6];
    if ( uvs ) { for ( int k = 0; k < 6; ++k ) u[k] = uvs[6 * ( size_t ) t + k]; }
    else { const DevProps& q = sc.props[t]; u[0] = q.ta[0]; u[1] = q.ta[1]; u[2] = q.tb[0]; u[3] = q.tb[1]; u[4] = q.tc[0]; u[5] = q.tc[1]; }
    const double sx = ( double ) at.uv_scale[0], sy = ( double ) at.uv_scale[1], ox = ( double ) at.uv_offset[0], oy = ( double ) at.uv_offset[1];
    AtlasTri T;
    T.ax = ( double ) u[0] * sx + ox; T.ay = ( double ) u[1] * sy + oy;
    T.bx = ( double ) u[2] * sx + ox; T.by = ( double ) u[3] * sy + oy;
    T.cx = ( double ) u[4] * sx + ox; T.cy = ( double ) u[5] * sy + oy;
    T.area2 = ( T.bx - T.ax ) * ( T.cy - T.ay ) - ( T.by - T.ay ) * ( T.cx - T.ax );
    T.ok = isfinite ( T.ax ) && isfinite ( T.ay ) && isfinite ( T.bx ) && isfinite ( T.by ) && isfinite ( T.cx ) && isfinite ( T.cy ) && isfinite ( T.area2 ) && T.area2 != 0.0;
    return T;
}

// one edge of the outside rule: the closest point's parameter and squared distance
__device__ void edge_closest ( double px, double py, double ux, double uy, double vx, double vy, double& t, double& d2 ) {
    const double ex = vx - ux, ey = vy - uy;
    t = ( ( px - ux ) * ex + ( py - uy ) * ey ) / ( ex * ex + ey * ey );
    t = t < 0.0 ? 0.0 : ( t > 1.0 ? 1.0 : t );
    const double qx = ux + t * ex, qy = uy + t * ey;
    d2 = ( px - qx ) * ( px - qx ) + ( py - qy ) * ( py - qy );
}

// the header's rule for texel (x, y) and triangle T (T.ok): candidate or not; wb, wc, d2 of the point taken
__device__ bool atlas_candidate ( const AtlasTri& T, uint32_t x, uint32_t y, double margin, double& wb, double& wc, double& d2 ) {
    const double px = ( double ) x + 0.5, py = ( double ) y + 0.5;
    const double ea = ( T.cx - T.bx ) * ( py - T.by ) - ( T.cy - T.by ) * ( px - T.bx );
    const double eb = ( T.ax - T.cx ) * ( py - T.cy ) - ( T.ay - T.cy ) * ( px - T.cx );
    const double ec = ( T.bx - T.ax ) * ( py - T.ay ) - ( T.by - T.ay ) * ( px - T.ax );
    const bool inside = T.area2 < 0.0 ? ( -ea >= 0.0 && -eb >= 0.0 && -ec >= 0.0 ) : ( ea >= 0.0 && eb >= 0.0 && ec >= 0.0 );
    if ( inside ) { d2 = 0.0; wb = eb / T.area2; wc = ec / T.area2; return true; }
    if ( ! ( margin > 0.0 ) ) return false;
    double t; int edge = 0;
    edge_closest ( px, py, T.ax, T.ay, T.bx, T.by, t, d2 );
    double tb, db; edge_closest ( px, py, T.bx, T.by, T.cx, T.cy, tb, db );
    if ( db < d2 ) { d2 = db; t = tb; edge = 1; }
    edge_closest ( px, py, T.cx, T.cy, T.ax, T.ay, tb, db );
    if ( db < d2 ) { d2 = db; t = tb; edge = 2; }
    if ( edge == 0 ) { wb = t; wc = 0.0; }
    else if ( edge == 1 ) { wb = 1.0 - t; wc = t; }
    else { wb = 0.0; wc = 1.0 - t; }
    return d2 <= margin * margin;
}

// one wave per triangle. The walked box is the exact one grown by at least half a texel on every side (rounding in the edge values can make a centre just outside the
// exact box a candidate; such a centre lies within rounding of it), and the whole atlas where a coordinate is so large that "within rounding" is not within half a texel
__global__ __launch_bounds__ ( 256 ) void terra_atlas_coverage ( DevScene sc, DevAtlas at, const float* uvs, unsigned long long* keys ) {
    const uint32_t t = __builtin_amdgcn_readfirstlane ( blockIdx.x * 4u + threadIdx.x / 64u );
    if ( t >= sc.n_tris ) return;
    const AtlasTri T = atlas_tri ( sc, at, uvs, t );
    if ( !T.ok ) return;
    const double m = ( double ) at.margin, w1 = ( double ) ( at.width - 1u ), h1 = ( double ) ( at.height - 1u );
    double x0 = floor ( fmin ( fmin ( T.ax, T.bx ), T.cx ) - m - 1.0 ), x1 = ceil ( fmax ( fmax ( T.ax, T.bx ), T.cx ) + m );
    double y0 = floor ( fmin ( fmin ( T.ay, T.by ), T.cy ) - m - 1.0 ), y1 = ceil ( fmax ( fmax ( T.ay, T.by ), T.cy ) + m );
    const double big = fmax ( fmax ( fmax ( fabs ( T.ax ), fabs ( T.ay ) ), fmax ( fabs ( T.bx ), fabs ( T.by ) ) ), fmax ( fabs ( T.cx ), fabs ( T.cy ) ) );
    if ( big > 1099511627776.0 ) { x0 = 0.0; y0 = 0.0; x1 = w1; y1 = h1; }          // 2^40
    x0 = fmax ( x0, 0.0 ); y0 = fmax ( y0, 0.0 ); x1 = fmin ( x1, w1 ); y1 = fmin ( y1, h1 );
    if ( x0 > x1 || y0 > y1 ) return;
    const uint32_t bx0 = ( uint32_t ) x0, by0 = ( uint32_t ) y0, bx1 = ( uint32_t ) x1, by1 = ( uint32_t ) y1;          // 0 <= b?0 <= b?1 <= size - 1
    const uint32_t tiles_x = ( bx1 - bx0 ) / 8u + 1u, tiles = tiles_x * ( ( by1 - by0 ) / 8u + 1u );
    const uint32_t lane = threadIdx.x & 63u, lx = lane & 7u, ly = lane >> 3;
    for ( uint32_t k = 0; k < tiles; ++k ) {          // (wave-uniform: every lane makes the same trips)
        const uint32_t x = bx0 + ( k % tiles_x ) * 8u + lx, y = by0 + ( k / tiles_x ) * 8u + ly;
        if ( x > bx1 || y > by1 ) continue;
        double wb, wc, d2;
        if ( !atlas_candidate ( T, x, y, m, wb, wc, d2 ) ) continue;
        const unsigned long long key = ( unsigned long long ) __float_as_uint ( ( float ) d2 ) << 32 | t;
        atomicMin ( &keys[ ( size_t ) y * at.width + x], key );
    }
}

__global__ __launch_bounds__ ( 256 ) void terra_atlas_resolve ( DevScene sc, DevAtlas at, const float* uvs, const unsigned long long* keys, float4* points, float4* texels ) {
    const size_t i = ( size_t ) blockIdx.x * 256u + threadIdx.x, n = ( size_t ) at.width * at.height;
    if ( i >= n ) return;
    const unsigned long long key = keys[i];
    float4 p0 = make_float4 ( 0.f, 0.f, 0.f, 0.f ), p1 = p0, rec = make_float4 ( __int_as_float ( -1 ), 0.f, 0.f, 0.f );
    if ( key != ~0ull ) {
        const uint32_t t = ( uint32_t ) key;
        const AtlasTri T = atlas_tri ( sc, at, uvs, t );
        double wb, wc, d2;
        atlas_candidate ( T, ( uint32_t ) ( i % at.width ), ( uint32_t ) ( i / at.width ), ( double ) at.margin, wb, wc, d2 );
        const double wa = ( 1.0 - wb ) - wc;
        const DevTri& v = sc.tris[t]; const DevProps& q = sc.props[t];
        auto mix = [&] ( float a, float b, float c ) { return ( float ) ( ( wa * ( double ) a + wb * ( double ) b ) + wc * ( double ) c ); };
        p0 = make_float4 ( mix ( v.a[0], v.b[0], v.c[0] ), mix ( v.a[1], v.b[1], v.c[1] ), mix ( v.a[2], v.b[2], v.c[2] ), 0.f );
        p1 = make_float4 ( mix ( q.na[0], q.nb[0], q.nc[0] ), mix ( q.na[1], q.nb[1], q.nc[1] ), mix ( q.na[2], q.nb[2], q.nc[2] ), 0.f );
        rec = make_float4 ( __int_as_float ( ( int ) t ), ( float ) wb, ( float ) wc, ( float ) d2 );
    }
    points[2 * i] = p0; points[2 * i + 1] = p1;
    if ( texels ) texels[i] = rec;
}

// one pass: every texel of (src, vsrc) to (dst, vdst); a valid texel as it is, an invalid one the mean of its valid neighbours
template <int CH>
__global__ __launch_bounds__ ( 256 ) void terra_dilate_pass ( const float* src, const int* vsrc, float* dst, int* vdst, uint32_t w, uint32_t h ) {
    const size_t i = ( size_t ) blockIdx.x * 256u + threadIdx.x;
    if ( i >= ( size_t ) w * h ) return;
    const int x = ( int ) ( i % w ), y = ( int ) ( i / w );
    float v[CH];
    for ( int c = 0; c < CH; ++c ) v[c] = src[i * CH + c];
    int valid = vsrc[i];
    if ( !valid ) {
        float sum[CH]; int count = 0;
        for ( int dy = -1; dy <= 1; ++dy ) for ( int dx = -1; dx <= 1; ++dx ) {
            if ( ( dx == 0 && dy == 0 ) || x + dx < 0 || y + dy < 0 || x + dx >= ( int ) w || y + dy >= ( int ) h ) continue;
            const size_t j = ( size_t ) ( y + dy ) * w + ( size_t ) ( x + dx );
            if ( !vsrc[j] ) continue;
            for ( int c = 0; c < CH; ++c ) sum[c] = count ? sum[c] + src[j * CH + c] : src[j * CH + c];
            ++count;
        }
        if ( count ) { for ( int c = 0; c < CH; ++c ) v[c] = sum[c] / ( float ) count; valid = 1; }
    }
    for ( int c = 0; c < CH; ++c ) dst[i * CH + c] = v[c];
    vdst[i] = valid;
}

}  // namespace

hipError_t terra_launch_atlas_points ( const DevScene& sc, const DevAtlas& atlas, const float* uvs, void* points, void* texels, hipStream_t stream ) {
    const size_t n = ( size_t ) atlas.width * atlas.height;
    unsigned long long* keys = nullptr;
    hipError_t e = hipMallocAsync ( ( void** ) &keys, n * sizeof ( unsigned long long ), stream );
    if ( e != hipSuccess ) return e;
    e = hipMemsetAsync ( keys, 0xff, n * sizeof ( unsigned long long ), stream );
    if ( e == hipSuccess && sc.n_tris ) {
        hipLaunchKernelGGL ( terra_atlas_coverage, dim3 ( ( sc.n_tris + 3u ) / 4u ), dim3 ( 256 ), 0, stream, sc, atlas, uvs, keys );
        e = hipGetLastError();
    }
    if ( e == hipSuccess ) {
        hipLaunchKernelGGL ( terra_atlas_resolve, dim3 ( ( uint32_t ) ( ( n + 255 ) / 256 ) ), dim3 ( 256 ), 0, stream, sc, atlas, uvs, keys, ( float4* ) points, ( float4* ) texels );
        e = hipGetLastError();
    }
    ( void ) hipFreeAsync ( keys, stream );
    return e;
}

hipError_t terra_launch_dilate ( float* data, int channels, int* valid, uint32_t width, uint32_t height, int passes, hipStream_t stream ) {
    if ( passes <= 0 ) return hipSuccess;
    const size_t n = ( size_t ) width * height, data_bytes = n * ( size_t ) channels * sizeof ( float ), data_room = ( data_bytes + 255 ) & ~ ( size_t ) 255;
    char* scratch = nullptr;
    hipError_t e = hipMallocAsync ( ( void** ) &scratch, data_room + n * sizeof ( int ), stream );
    if ( e != hipSuccess ) return e;
    float* d[2] = { data, ( float* ) scratch }; int* v[2] = { valid, ( int* ) ( scratch + data_room ) };
    const dim3 grid ( ( uint32_t ) ( ( n + 255 ) / 256 ) ), block ( 256 );
    for ( int k = 0; k < passes && e == hipSuccess; ++k ) {
        const int a = k & 1, b = a ^ 1;
        switch ( channels ) {
            case 1: hipLaunchKernelGGL ( terra_dilate_pass<1>, grid, block, 0, stream, d[a], v[a], d[b], v[b], width, height ); break;
            case 2: hipLaunchKernelGGL ( terra_dilate_pass<2>, grid, block, 0, stream, d[a], v[a], d[b], v[b], width, height ); break;
            case 3: hipLaunchKernelGGL ( terra_dilate_pass<3>, grid, block, 0, stream, d[a], v[a], d[b], v[b], width, height ); break;
            default: hipLaunchKernelGGL ( terra_dilate_pass<4>, grid, block, 0, stream, d[a], v[a], d[b], v[b], width, height ); break;
        }
        e = hipGetLastError();
    }
    if ( e == hipSuccess && ( passes & 1 ) ) {          // an odd number of passes ends in the second copy
        e = hipMemcpyAsync ( data, d[1], data_bytes, hipMemcpyDeviceToDevice, stream );
        if ( e == hipSuccess ) e = hipMemcpyAsync ( valid, v[1], n * sizeof ( int ), hipMemcpyDeviceToDevice, stream );
    }
    ( void ) hipFreeAsync ( scratch, stream );
    return e;
}
