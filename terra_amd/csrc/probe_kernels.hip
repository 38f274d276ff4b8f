// probe_kernels.hip -- probe harmonics (include/terra_amd.h "Probe harmonics" is the definition): the rays of a probe frame, the reduction of a rendered
// probe frame to order-2 real spherical harmonics, and irradiance from those. Three kernels:
//   terra_probe_rays      one lane per ray: the cell's stratified pair, then point_sample (trace_geometry.h, distribution 1) about the probe -- the record
//                         terra_unit_point_rays gives; two 16-byte stores
//   terra_sh_project      one wave per probe, four waves per block: lanes read consecutive cells (one 16-byte load of the result, two of the ray), 27 binary64
//                         accumulators per lane, six shuffle steps in the header's order, lane 0 writes the record. No atomics
//   terra_sh_irradiance   one lane per query: the probe's coefficients, or the grid's eight corners blended in the header's order, against the cosine lobe
// and probe visibility (include/terra_amd.h "Probe visibility"), two kernels, described where they stand:
//   terra_visibility_project      one wave per probe: the hit distances of a probe frame filtered into an octahedral map of distance moments
//   terra_sh_irradiance_visible   one lane per query: the grid blend with every probe weighted by a Chebyshev test against its map and a back-face term
// Everything of rules 2 and 3 and of probe visibility is binary64 (the unit is built with -ffp-contract=off like the others; binary64 division is IEEE, the square root is the _rn form).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "trace_geometry.h"
#include "kernels.h"

namespace {

// the ray door's rule for a record that traces nothing: a direction of exactly (0, 0, 0), or an origin or direction component that is not finite
__device__ bool ray_inactive ( const float4& o, const float4& d ) {
    const bool finite = fabsf ( o.x ) < INFINITY && fabsf ( o.y ) < INFINITY && fabsf ( o.z ) < INFINITY && fabsf ( d.x ) < INFINITY && fabsf ( d.y ) < INFINITY && fabsf ( d.z ) < INFINITY;      // (false for a NaN too)
    return !finite || ( d.x == 0.f && d.y == 0.f && d.z == 0.f );
}

// the nine basis values of the direction (x, y, z), used as given
__device__ __forceinline__ void sh_basis ( double x, double y, double z, double* Y ) {
    Y[0] = 0.28209479177387814;
    Y[1] = 0.4886025119029199 * y;
    Y[2] = 0.4886025119029199 * z;
    Y[3] = 0.4886025119029199 * x;
    Y[4] = 1.0925484305920792 * ( x * y );
    Y[5] = 1.0925484305920792 * ( y * z );
    Y[6] = 0.31539156525252005 * ( ( 3.0 * ( z * z ) ) - 1.0 );
    Y[7] = 1.0925484305920792 * ( x * z );
    Y[8] = 0.5462742152960396 * ( ( x * x ) - ( y * y ) );
}

// the cosine lobe about the unit direction (x, y, z) against the 27 coefficients c[3 * k + channel]: (E_r, E_g, E_b, 0)
__device__ __forceinline__ float4 sh_lobe ( const double* c, double x, double y, double z ) {
    double Y[9]; sh_basis ( x, y, z, Y );
    double E[3];
#pragma unroll
    for ( int k = 0; k < 9; ++k ) {
        const double A = k == 0 ? 3.141592653589793 : ( k < 4 ? 2.0943951023931953 : 0.7853981633974483 );
#pragma unroll
        for ( int ch = 0; ch < 3; ++ch ) { const double term = ( A * c[3 * k + ch] ) * Y[k]; E[ch] = k ? E[ch] + term : term; }
    }
    return make_float4 ( ( float ) E[0], ( float ) E[1], ( float ) E[2], 0.f );
}

// a cell's pair on one axis: ((float) i + j) / (float) n, a NaN or a negative value to 0, anything above 1 - 2^-24 to that
__device__ __forceinline__ float cell_coordinate ( uint32_t i, float j, uint32_t n ) {
    float g = ( ( float ) i + j ) / ( float ) n;
    if ( ! ( g >= 0.f ) ) g = 0.f;
    if ( g > 0.99999994f ) g = 0.99999994f;          // 1 - 2^-24 = 0x3F7FFFFF
    return g;
}

__global__ __launch_bounds__ ( 256 ) void terra_probe_rays ( const float4* probes, const float* jitter, float4* rays, uint32_t total, uint32_t n, uint32_t K ) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if ( r >= total ) return;
    const uint32_t p = r / K, c = r - p * K, j = c / n, i = c - j * n;
    const float4 q0 = probes[2 * ( size_t ) p], q1 = probes[2 * ( size_t ) p + 1];
    const V3 pos = v3 ( q0.x, q0.y, q0.z ), nrm = v3 ( q1.x, q1.y, q1.z );
    float4 o = make_float4 ( 0.f, 0.f, 0.f, 0.f ), d = o;
    if ( !point_inactive ( pos, nrm ) ) {
        const float ju = jitter ? jitter[2 * c] : 0.5f, jv = jitter ? jitter[2 * c + 1] : 0.5f;
        DevPointSampling S; S.distribution = 1;
        V3 ro, rd;
        point_sample ( S, pos, nrm, cell_coordinate ( i, ju, n ), cell_coordinate ( j, jv, n ), ro, rd );
        o = make_float4 ( ro.x, ro.y, ro.z, FLT_MAX ); d = make_float4 ( rd.x, rd.y, rd.z, 0.f );
    }
    rays[2 * ( size_t ) r] = o; rays[2 * ( size_t ) r + 1] = d;
}

__global__ __launch_bounds__ ( 256 ) void terra_sh_project ( const float4* results, const float4* rays, float4* sh, uint32_t probes, uint32_t K, int batch ) {
    const uint32_t p = __builtin_amdgcn_readfirstlane ( blockIdx.x * 4u + threadIdx.x / 64u );
    if ( p >= probes ) return;
    const float4* res = results + ( size_t ) p * K;
    const float4* ray = rays + 2 * ( size_t ) p * K;
    const uint32_t lane = threadIdx.x & 63u;
    double acc[27];
#pragma unroll
    for ( int k = 0; k < 27; ++k ) acc[k] = 0.0;
    int count = 0;
    for ( uint32_t c = lane; c < K; c += 64u ) {
        const float4 r = res[c], o = ray[2 * ( size_t ) c], d = ray[2 * ( size_t ) c + 1];
        const int samples = __float_as_int ( r.w );
        if ( samples <= 0 || ray_inactive ( o, d ) ) continue;
        const double L[3] = { ( double ) r.x / ( double ) samples, ( double ) r.y / ( double ) samples, ( double ) r.z / ( double ) samples };
        double Y[9]; sh_basis ( ( double ) d.x, ( double ) d.y, ( double ) d.z, Y );
#pragma unroll
        for ( int k = 0; k < 9; ++k ) {
#pragma unroll
            for ( int ch = 0; ch < 3; ++ch ) acc[3 * k + ch] = acc[3 * k + ch] + L[ch] * Y[k];
        }
        ++count;
    }
    // partial[l] = partial[l] + partial[l + s] for l < s, s = 32 .. 1 (a lane at or beyond s adds something nobody reads)
#pragma unroll
    for ( int s = 32; s >= 1; s >>= 1 ) {
#pragma unroll
        for ( int k = 0; k < 27; ++k ) acc[k] = acc[k] + __shfl_down ( acc[k], s, 64 );
        count += __shfl_down ( count, s, 64 );
    }
    if ( lane != 0 ) return;
    float4* out = sh + 7 * ( size_t ) p;
    const double scale = 12.566370614359172 / ( double ) K;
    float w[28];
    if ( batch > 0 ) {
#pragma unroll
        for ( int k = 0; k < 7; ++k ) { const float4 v = out[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
    }
#pragma unroll
    for ( int k = 0; k < 27; ++k ) {
        const double fresh = acc[k] * scale;
        w[k] = batch > 0 ? ( float ) ( ( ( ( double ) w[k] * ( double ) batch ) + fresh ) / ( double ) ( batch + 1 ) ) : ( float ) fresh;
    }
    w[27] = __int_as_float ( count );
#pragma unroll
    for ( int k = 0; k < 7; ++k ) out[k] = make_float4 ( w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3] );
}

// one axis of the grid lookup: the lower probe, the upper one and the weight of the upper; false for a NaN
__device__ __forceinline__ bool grid_axis ( float pos, float origin, float spacing, int count, int& lo, int& hi, double& t ) {
    double f = ( ( double ) pos - ( double ) origin ) / ( double ) spacing;
    if ( f != f ) return false;
    const double top = ( double ) ( count - 1 );
    if ( f < 0.0 ) f = 0.0;
    if ( f > top ) f = top;
    lo = ( int ) floor ( f );
    const int last = count - 2 > 0 ? count - 2 : 0;
    if ( lo > last ) lo = last;
    t = f - ( double ) lo;
    hi = lo + 1 < count - 1 ? lo + 1 : count - 1;
    return true;
}

__global__ __launch_bounds__ ( 256 ) void terra_sh_irradiance ( const float4* sh, uint32_t probes, DevProbeGrid grid, const float4* points, const int* index, uint32_t n, float4* out ) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if ( i >= n ) return;
    const float4 zero = make_float4 ( 0.f, 0.f, 0.f, 0.f );
    const float4 q0 = points[2 * ( size_t ) i], q1 = points[2 * ( size_t ) i + 1];
    const double nx = ( double ) q1.x, ny = ( double ) q1.y, nz = ( double ) q1.z;
    const double q = ( nx * nx + ny * ny ) + nz * nz;
    const bool finite = fabsf ( q1.x ) < INFINITY && fabsf ( q1.y ) < INFINITY && fabsf ( q1.z ) < INFINITY;
    if ( !finite || ! ( q > 0.0 && q < ( double ) INFINITY ) ) { out[i] = zero; return; }
    const double len = __dsqrt_rn ( q );
    double c[27];
    if ( grid.on ) {
        int lo[3], hi[3]; double t[3];
        if ( !grid_axis ( q0.x, grid.origin[0], grid.spacing[0], grid.count[0], lo[0], hi[0], t[0] ) || !grid_axis ( q0.y, grid.origin[1], grid.spacing[1], grid.count[1], lo[1], hi[1], t[1] ) ||
             !grid_axis ( q0.z, grid.origin[2], grid.spacing[2], grid.count[2], lo[2], hi[2], t[2] ) ) { out[i] = zero; return; }
#pragma unroll
        for ( int corner = 0; corner < 8; ++corner ) {
            const int dz = corner >> 2, dy = ( corner >> 1 ) & 1, dx = corner & 1;
            const double wz = dz ? t[2] : 1.0 - t[2], wy = dy ? t[1] : 1.0 - t[1], wx = dx ? t[0] : 1.0 - t[0];
            const double weight = ( wz * wy ) * wx;
            const size_t probe = ( ( size_t ) ( dz ? hi[2] : lo[2] ) * ( size_t ) grid.count[1] + ( size_t ) ( dy ? hi[1] : lo[1] ) ) * ( size_t ) grid.count[0] + ( size_t ) ( dx ? hi[0] : lo[0] );
            const float4* rec = sh + 7 * probe;
#pragma unroll
            for ( int k = 0; k < 7; ++k ) {
                const float4 v = rec[k];
                const float f[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                for ( int m = 0; m < 4; ++m ) if ( 4 * k + m < 27 ) c[4 * k + m] = corner ? c[4 * k + m] + weight * ( double ) f[m] : weight * ( double ) f[m];
            }
        }
    } else {
        const int at = index[i];
        if ( at < 0 || ( uint32_t ) at >= probes ) { out[i] = zero; return; }
        const float4* rec = sh + 7 * ( size_t ) at;
#pragma unroll
        for ( int k = 0; k < 7; ++k ) {
            const float4 v = rec[k];
            const float f[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for ( int m = 0; m < 4; ++m ) if ( 4 * k + m < 27 ) c[4 * k + m] = ( double ) f[m];
        }
    }
    out[i] = sh_lobe ( c, nx / len, ny / len, nz / len );
}

// ---- probe visibility (include/terra_amd.h "Probe visibility" is the definition) ------------------------------------------------------------------
__device__ __forceinline__ double sgn ( double x ) { return x >= 0.0 ? 1.0 : -1.0; }

// one wave per probe, four waves per block. Lane l owns the texels l, l + 64, l + 128, l + 192 (those below m * m): their directions are made once, their three sums
// are chains over the cells in ascending order. The cells go through a per-wave slice of LDS 64 at a time: every lane reduces one cell to (rx, ry, rz, d, d * d) --
// a cell that takes no part gets a NaN direction, which no texel adds, as !(cosv > 0) says -- and the loop then reads one address per step (a broadcast). A lane's
// spare texel has the direction (0, 0, 0): cosv is 0 or NaN, nothing is added. A wave without a probe does no work but meets every barrier.
__global__ __launch_bounds__ ( 256 ) void terra_visibility_project ( const float4* hits, const float4* rays, float4* map, uint32_t probes, uint32_t K, uint32_t m, int sharpness,
                                                                      float max_distance, int accumulate ) {
    __shared__ __attribute__ ( ( aligned ( 16 ) ) ) double stage[4][64][6];          // (five used; 48 bytes a cell keeps the 16-byte reads aligned)
    const uint32_t wave = __builtin_amdgcn_readfirstlane ( threadIdx.x / 64u );
    const uint32_t p = __builtin_amdgcn_readfirstlane ( blockIdx.x * 4u + wave );
    const bool live = p < probes;
    const uint32_t lane = threadIdx.x & 63u, mm = m * m;
    const float4* hit = hits + 2 * ( size_t ) ( live ? p : 0u ) * K;
    const float4* ray = rays + 2 * ( size_t ) ( live ? p : 0u ) * K;
    double Tx[4], Ty[4], Tz[4], W[4], Wd[4], Wd2[4];
    int added[4];
#pragma unroll
    for ( int q = 0; q < 4; ++q ) {
        const uint32_t t = lane + 64u * ( uint32_t ) q;
        Tx[q] = 0.0; Ty[q] = 0.0; Tz[q] = 0.0; W[q] = 0.0; Wd[q] = 0.0; Wd2[q] = 0.0; added[q] = 0;
        if ( t < mm ) {
            const uint32_t j = t / m, i = t - j * m;
            const double qx = ( 2.0 * ( ( ( double ) i + 0.5 ) / ( double ) m ) ) - 1.0, qy = ( 2.0 * ( ( ( double ) j + 0.5 ) / ( double ) m ) ) - 1.0;
            const double z = ( 1.0 - fabs ( qx ) ) - fabs ( qy );
            const double x = z < 0.0 ? ( 1.0 - fabs ( qy ) ) * sgn ( qx ) : qx, y = z < 0.0 ? ( 1.0 - fabs ( qx ) ) * sgn ( qy ) : qy;
            const double len = __dsqrt_rn ( ( ( x * x ) + ( y * y ) ) + ( z * z ) );
            Tx[q] = x / len; Ty[q] = y / len; Tz[q] = z / len;
        }
    }
    const double cap = ( double ) max_distance;
    for ( uint32_t base = 0; base < K; base += 64u ) {
        const uint32_t c = base + lane;
        if ( live && c < K ) {
            const float4 h = hit[2 * ( size_t ) c], o = ray[2 * ( size_t ) c], d = ray[2 * ( size_t ) c + 1];
            double dist = __float_as_int ( h.y ) < 0 ? cap : ( double ) h.x;
            if ( ! ( h.x <= max_distance ) ) dist = cap;
            const bool off = ray_inactive ( o, d );
            double* cell = stage[wave][lane];
            cell[0] = off ? ( double ) NAN : ( double ) d.x; cell[1] = ( double ) d.y; cell[2] = ( double ) d.z; cell[3] = dist; cell[4] = dist * dist;
        }
        __syncthreads();
        if ( live ) {
            const uint32_t count = K - base < 64u ? K - base : 64u;
            for ( uint32_t k = 0; k < count; ++k ) {
                const double* cell = stage[wave][k];
                const double rx = cell[0], ry = cell[1], rz = cell[2], dist = cell[3], dist2 = cell[4];
#pragma unroll
                for ( int q = 0; q < 4; ++q ) {
                    if ( 64u * ( uint32_t ) q < mm ) {          // (uniform: a map of up to 64 texels has one per lane)
                        const double cosv = ( ( Tx[q] * rx ) + ( Ty[q] * ry ) ) + ( Tz[q] * rz );
                        double w = cosv;
                        for ( int s = 0; s < sharpness; ++s ) w = w * w;
                        const bool on = cosv > 0.0;
                        w = on ? w : 0.0;          // (the sums are +0 or above and d is finite: adding +0 changes no bit, so a cell passed over needs no branch)
                        W[q] = W[q] + w; Wd[q] = Wd[q] + ( w * dist ); Wd2[q] = Wd2[q] + ( w * dist2 );
                        added[q] += on ? 1 : 0;
                    }
                }
            }
        }
        __syncthreads();
    }
    if ( !live ) return;
    float4* out = map + ( size_t ) p * mm;
#pragma unroll
    for ( int q = 0; q < 4; ++q ) {
        const uint32_t t = lane + 64u * ( uint32_t ) q;
        if ( t >= mm ) continue;
        float4 v = make_float4 ( ( float ) W[q], ( float ) Wd[q], ( float ) Wd2[q], __int_as_float ( added[q] ) );
        if ( accumulate ) {
            const float4 old = out[t];
            v = make_float4 ( ( float ) ( ( double ) old.x + W[q] ), ( float ) ( ( double ) old.y + Wd[q] ), ( float ) ( ( double ) old.z + Wd2[q] ),
                              __int_as_float ( ( int ) ( ( uint32_t ) __float_as_int ( old.w ) + ( uint32_t ) added[q] ) ) );
        }
        out[t] = v;
    }
}

// the octahedral wrap of a tap, then its record
__device__ __forceinline__ float4 visibility_tap ( const float4* texels, int i, int j, int m ) {
    if ( i < 0 ) { i = 0; j = m - 1 - j; } else if ( i >= m ) { i = m - 1; j = m - 1 - j; }
    if ( j < 0 ) { j = 0; i = m - 1 - i; } else if ( j >= m ) { j = m - 1; i = m - 1 - i; }
    return texels[j * m + i];
}

// the Chebyshev term of one probe for the offset V of length dist (> 0 and finite): the map's three sums blended over four taps, then the one-sided bound
__device__ double visibility_weight ( const float4* texels, int m, double Vx, double Vy, double Vz, double a, double dist ) {
    double px = Vx / a, py = Vy / a;
    if ( Vz < 0.0 ) { const double ox = px, oy = py; px = ( 1.0 - fabs ( oy ) ) * sgn ( ox ); py = ( 1.0 - fabs ( ox ) ) * sgn ( oy ); }
    const double u = ( px * 0.5 ) + 0.5, v = ( py * 0.5 ) + 0.5;
    const double fx = ( u * ( double ) m ) - 0.5, fy = ( v * ( double ) m ) - 0.5;
    const double x0 = floor ( fx ), y0 = floor ( fy ), tx = fx - x0, ty = fy - y0;
    const int i0 = ( int ) x0, j0 = ( int ) y0;          // (u, v in [0, 1]: -1 .. m - 1)
    double W = 0.0, Wd = 0.0, Wd2 = 0.0;
#pragma unroll
    for ( int tap = 0; tap < 4; ++tap ) {
        const int dj = tap >> 1, di = tap & 1;
        const double weight = ( dj ? ty : 1.0 - ty ) * ( di ? tx : 1.0 - tx );
        const float4 r = visibility_tap ( texels, i0 + di, j0 + dj, m );
        W = tap ? W + weight * ( double ) r.x : weight * ( double ) r.x;
        Wd = tap ? Wd + weight * ( double ) r.y : weight * ( double ) r.y;
        Wd2 = tap ? Wd2 + weight * ( double ) r.z : weight * ( double ) r.z;
    }
    if ( ! ( W > 0.0 ) ) return 1.0;
    const double mean = Wd / W, mean2 = Wd2 / W, var = fabs ( ( mean * mean ) - mean2 );
    if ( dist <= mean ) return 1.0;
    const double e = dist - mean, q = var + ( e * e );
    if ( ! ( q > 0.0 ) ) return 0.0;
    const double ch = var / q;
    return ( ch * ch ) * ch;
}

// one lane per query: terra_sh_irradiance's grid arm with every corner's weight multiplied by the back-face and the visibility term, the plain sums kept beside
__global__ __launch_bounds__ ( 256 ) void terra_sh_irradiance_visible ( const float4* sh, const float4* map, DevProbeGrid grid, DevProbeVisibility opt, const float4* points, uint32_t n, float4* out ) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if ( i >= n ) return;
    const float4 zero = make_float4 ( 0.f, 0.f, 0.f, 0.f );
    const float4 q0 = points[2 * ( size_t ) i], q1 = points[2 * ( size_t ) i + 1];
    const double nx = ( double ) q1.x, ny = ( double ) q1.y, nz = ( double ) q1.z;
    const double q = ( nx * nx + ny * ny ) + nz * nz;
    const bool finite = fabsf ( q1.x ) < INFINITY && fabsf ( q1.y ) < INFINITY && fabsf ( q1.z ) < INFINITY;
    if ( !finite || ! ( q > 0.0 && q < ( double ) INFINITY ) ) { out[i] = zero; return; }
    const double len = __dsqrt_rn ( q );
    const double N[3] = { nx / len, ny / len, nz / len };
    int lo[3], hi[3]; double t[3];
    if ( !grid_axis ( q0.x, grid.origin[0], grid.spacing[0], grid.count[0], lo[0], hi[0], t[0] ) || !grid_axis ( q0.y, grid.origin[1], grid.spacing[1], grid.count[1], lo[1], hi[1], t[1] ) ||
         !grid_axis ( q0.z, grid.origin[2], grid.spacing[2], grid.count[2], lo[2], hi[2], t[2] ) ) { out[i] = zero; return; }
    const double bias = ( double ) opt.bias;
    const double X[3] = { ( double ) q0.x + ( bias * N[0] ), ( double ) q0.y + ( bias * N[1] ), ( double ) q0.z + ( bias * N[2] ) };
    const int m = opt.texels;
    double plain[27], c[27], S = 0.0;
    for ( int corner = 0; corner < 8; ++corner ) {
        const int dz = corner >> 2, dy = ( corner >> 1 ) & 1, dx = corner & 1;
        const double wz = dz ? t[2] : 1.0 - t[2], wy = dy ? t[1] : 1.0 - t[1], wx = dx ? t[0] : 1.0 - t[0];
        const double wt = ( wz * wy ) * wx;
        const int at[3] = { dx ? hi[0] : lo[0], dy ? hi[1] : lo[1], dz ? hi[2] : lo[2] };
        const size_t probe = ( ( size_t ) at[2] * ( size_t ) grid.count[1] + ( size_t ) at[1] ) * ( size_t ) grid.count[0] + ( size_t ) at[0];
        double V[3];
#pragma unroll
        for ( int a = 0; a < 3; ++a ) V[a] = X[a] - ( double ) ( float ) ( ( double ) grid.origin[a] + ( double ) at[a] * ( double ) grid.spacing[a] );
        const double dist = __dsqrt_rn ( ( ( V[0] * V[0] ) + ( V[1] * V[1] ) ) + ( V[2] * V[2] ) );
        double wb = 1.0;
        if ( opt.backface ) {
            wb = 1.2;
            if ( dist > 0.0 ) { const double bf = ( ( ( ( - ( ( V[0] * N[0] ) + ( V[1] * N[1] ) ) ) - ( V[2] * N[2] ) ) / dist ) + 1.0 ) * 0.5; wb = ( bf * bf ) + 0.2; }
        }
        const double a = ( fabs ( V[0] ) + fabs ( V[1] ) ) + fabs ( V[2] );
        double wv = 1.0;
        if ( dist != 0.0 && a < ( double ) INFINITY ) wv = visibility_weight ( map + probe * ( size_t ) ( m * m ), m, V[0], V[1], V[2], a, dist );
        const double w = ( wt * wb ) * wv;
        S = corner ? S + w : w;
        const float4* rec = sh + 7 * probe;
#pragma unroll
        for ( int k = 0; k < 7; ++k ) {
            const float4 v = rec[k];
            const float f[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for ( int e = 0; e < 4; ++e ) if ( 4 * k + e < 27 ) {
                plain[4 * k + e] = corner ? plain[4 * k + e] + wt * ( double ) f[e] : wt * ( double ) f[e];
                c[4 * k + e] = corner ? c[4 * k + e] + w * ( double ) f[e] : w * ( double ) f[e];
            }
        }
    }
    const bool seen = S > 0.0;
#pragma unroll
    for ( int k = 0; k < 27; ++k ) c[k] = seen ? c[k] / S : plain[k];
    out[i] = sh_lobe ( c, N[0], N[1], N[2] );
}

}  // namespace

hipError_t terra_launch_probe_rays ( const void* probes, uint32_t count, uint32_t cells, const float* jitter, void* rays, hipStream_t stream ) {
    const uint32_t K = cells * cells, total = count * K;          // (the host layer keeps K * P within 2^31 - 1)
    if ( !total ) return hipSuccess;
    hipLaunchKernelGGL ( terra_probe_rays, dim3 ( ( total + 255u ) / 256u ), dim3 ( 256 ), 0, stream, ( const float4* ) probes, jitter, ( float4* ) rays, total, cells, K );
    return hipGetLastError();
}

hipError_t terra_launch_sh_project ( const void* results, const void* rays, uint32_t count, uint32_t cells, int batch, void* sh, hipStream_t stream ) {
    if ( !count ) return hipSuccess;
    hipLaunchKernelGGL ( terra_sh_project, dim3 ( ( count + 3u ) / 4u ), dim3 ( 256 ), 0, stream, ( const float4* ) results, ( const float4* ) rays, ( float4* ) sh, count, cells * cells, batch );
    return hipGetLastError();
}

hipError_t terra_launch_sh_irradiance ( const void* sh, uint32_t probes, const DevProbeGrid& grid, const void* points, const int* index, uint32_t n, void* out, hipStream_t stream ) {
    if ( !n ) return hipSuccess;
    hipLaunchKernelGGL ( terra_sh_irradiance, dim3 ( ( n + 255u ) / 256u ), dim3 ( 256 ), 0, stream, ( const float4* ) sh, probes, grid, ( const float4* ) points, index, n, ( float4* ) out );
    return hipGetLastError();
}

hipError_t terra_launch_probe_visibility ( const void* hits, const void* rays, uint32_t count, uint32_t cells, const DevProbeVisibility& options, int accumulate, void* map, hipStream_t stream ) {
    if ( !count ) return hipSuccess;
    hipLaunchKernelGGL ( terra_visibility_project, dim3 ( ( count + 3u ) / 4u ), dim3 ( 256 ), 0, stream, ( const float4* ) hits, ( const float4* ) rays, ( float4* ) map, count, cells * cells,
                         ( uint32_t ) options.texels, options.sharpness, options.max_distance, accumulate );
    return hipGetLastError();
}

hipError_t terra_launch_sh_irradiance_visible ( const void* sh, const void* map, const DevProbeGrid& grid, const DevProbeVisibility& options, const void* points, uint32_t n, void* out, hipStream_t stream ) {
    if ( !n ) return hipSuccess;
    hipLaunchKernelGGL ( terra_sh_irradiance_visible, dim3 ( ( n + 255u ) / 256u ), dim3 ( 256 ), 0, stream, ( const float4* ) sh, ( const float4* ) map, grid, options, ( const float4* ) points, n, ( float4* ) out );
    return hipGetLastError();
}
