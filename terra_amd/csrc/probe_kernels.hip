// probe_kernels.hip -- probe harmonics (include/terra_amd.h "Probe harmonics" is the definition): the rays of a probe frame, the reduction of a rendered
// probe frame to order-2 real spherical harmonics, and irradiance from those. Three kernels:
//   terra_probe_rays      one lane per ray: the cell's stratified pair, then point_sample (trace_geometry.h, distribution 1) about the probe -- the record
//                         terra_unit_point_rays gives; two 16-byte stores
//   terra_sh_project      one wave per probe, four waves per block: lanes read consecutive cells (one 16-byte load of the result, two of the ray), 27 binary64
//                         accumulators per lane, six shuffle steps in the header's order, lane 0 writes the record. No atomics
//   terra_sh_irradiance   one lane per query: the probe's coefficients, or the grid's eight corners blended in the header's order, against the cosine lobe
// Everything of rules 2 and 3 is binary64 (the unit is built with -ffp-contract=off like the others; binary64 division is IEEE, the square root is the _rn form).
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
    double Y[9]; sh_basis ( nx / len, ny / len, nz / len, Y );
    double E[3];
#pragma unroll
    for ( int k = 0; k < 9; ++k ) {
        const double A = k == 0 ? 3.141592653589793 : ( k < 4 ? 2.0943951023931953 : 0.7853981633974483 );
#pragma unroll
        for ( int ch = 0; ch < 3; ++ch ) { const double term = ( A * c[3 * k + ch] ) * Y[k]; E[ch] = k ? E[ch] + term : term; }
    }
    out[i] = make_float4 ( ( float ) E[0], ( float ) E[1], ( float ) E[2], 0.f );
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
