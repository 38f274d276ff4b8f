// unit_kernels.hip -- one-function-per-kernel wrappers over the device functions
// of trace_device.h, so parity tests can pin every stage of the path against the
// oracle and the golden vectors (include/terra_amd.h, "unit-level device entry points").
#include <hip/hip_runtime.h>
#include "trace_device.h"
#include "sampling_device.h"
#include "kernels.h"

#define UNIT_GRID(n) dim3 ( ( ( n ) + 255 ) / 256 ), dim3 ( 256 )

__global__ void k_pcg ( const uint32_t* seeds, int nseeds, int n, float* out ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= nseeds ) return;
    Pcg32 a; a.state = 0; a.inc = 1;
    trng_next ( a ); a.state += seeds[i]; trng_next ( a );
    for ( int j = 0; j < n; ++j ) out[ ( size_t ) i * n + j] = trng_a_float ( a );
}
hipError_t terra_unit_pcg ( const uint32_t* seeds, int nseeds, int n, float* out ) {
    hipLaunchKernelGGL ( k_pcg, UNIT_GRID ( nseeds ), 0, 0, seeds, nseeds, n, out );
    return hipGetLastError();
}

__global__ void k_stream_keys ( uint64_t seed, const uint64_t* pix, const uint64_t* k, int n, uint64_t* out3 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    PixelStreams s = trng_pixel_streams ( seed, pix[i], k[i] );
    out3[3 * i] = s.seedA; out3[3 * i + 1] = s.b.state; out3[3 * i + 2] = s.b.inc;
}
hipError_t terra_unit_stream_keys ( uint64_t frame_seed, const uint64_t* pix, const uint64_t* k, int n, uint64_t* out3 ) {
    hipLaunchKernelGGL ( k_stream_keys, UNIT_GRID ( n ), 0, 0, frame_seed, pix, k, n, out3 );
    return hipGetLastError();
}

__global__ void k_ray_aabb ( int n, const float* o, const float* d, const float* boxes, int* hit, float* tmin, float* tmax ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    Ray r = make_ray ( v3p ( o + 3 * i ), v3p ( d + 3 * i ) );
    float a, b;
    bool h = ray_aabb ( r, v3p ( boxes + 6 * i ), v3p ( boxes + 6 * i + 3 ), &a, &b );
    hit[i] = h ? 1 : 0;
    if ( h ) { tmin[i] = a; tmax[i] = b; }
}
hipError_t terra_unit_ray_aabb ( int n, const float* o, const float* d, const float* boxes, int* hit, float* tmin, float* tmax ) {
    hipLaunchKernelGGL ( k_ray_aabb, UNIT_GRID ( n ), 0, 0, n, o, d, boxes, hit, tmin, tmax );
    return hipGetLastError();
}

__global__ void k_watertight ( int n, const float* o, const float* d, const float* tris, int* hit, float* out8 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    Ray r = make_ray ( v3p ( o + 3 * i ), v3p ( d + 3 * i ) );
    RayState s = ray_state_init ( r );
    TriHit h; h.u = h.v = h.w = h.depth = 0.f; h.point = v3 ( 0, 0, 0 );
    bool ok = watertight ( r, s, v3p ( tris + 9 * i ), v3p ( tris + 9 * i + 3 ), v3p ( tris + 9 * i + 6 ), h );
    hit[i] = ok ? 1 : 0;
    float* q = out8 + 8 * i;
    if ( ok ) { q[0] = h.u; q[1] = h.v; q[2] = h.w; q[3] = h.depth; q[4] = h.point.x; q[5] = h.point.y; q[6] = h.point.z; q[7] = 0.f; }
    else { for ( int j = 0; j < 8; ++j ) q[j] = 0.f; }
}
hipError_t terra_unit_watertight ( int n, const float* o, const float* d, const float* tris, int* hit, float* out8 ) {
    hipLaunchKernelGGL ( k_watertight, UNIT_GRID ( n ), 0, 0, n, o, d, tris, hit, out8 );
    return hipGetLastError();
}

// watertight_pair on one fan per ray: quads = p0 p1 p2 p3 (12 floats); hit[2 i], hit[2 i + 1] and depth[2 i], depth[2 i + 1] for T1 = (p0, p1, p2) and T2 = (p0, p2, p3).
// Must equal k_watertight run on each triangle, bit for bit (tests/test_leaf_pairs_gpu.py)
__global__ void k_watertight_pair ( int n, const float* o, const float* d, const float* quads, int* hit, float* depth ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    // the ray start of the LDS-resident kernels (trace_geometry.h ray_start_masks): axes by lane predicates, ix / iy / iz from perm's tables, the origin picked with them
    bool guarded;
    Ray r = make_ray_guarded ( v3p ( o + 3 * i ), v3p ( d + 3 * i ), guarded );
    V3 o_perm;
    const RayStateMasks s = ray_start_masks ( r, o_perm );
    auto load = [&] ( bool again ) {
        const float* q = quads + 12 * i;
        if ( again ) asm volatile ( "" : "+v" ( q ) );
        const V3 p0 = v3p ( q ), p1 = v3p ( q + 3 ), p2 = v3p ( q + 6 ), p3 = v3p ( q + 9 );
        return PairPerm { { pick ( p0, s.ix ), pick ( p0, s.iy ), pick ( p0, s.iz ) }, { pick ( p1, s.ix ), pick ( p1, s.iy ), pick ( p1, s.iz ) },
                          { pick ( p2, s.ix ), pick ( p2, s.iy ), pick ( p2, s.iz ) }, { pick ( p3, s.ix ), pick ( p3, s.iy ), pick ( p3, s.iz ) } };
    };
    int h0 = 0, h1 = 0; float d0 = 0.f, d1 = 0.f;
    watertight_pair ( load, o_perm, s, [&] ( float dep, bool second ) { if ( second ) { h1 = 1; d1 = dep; } else { h0 = 1; d0 = dep; } } );
    hit[2 * i] = h0; hit[2 * i + 1] = h1; depth[2 * i] = d0; depth[2 * i + 1] = d1;
}
hipError_t terra_unit_watertight_pair ( int n, const float* o, const float* d, const float* quads, int* hit, float* depth ) {
    hipLaunchKernelGGL ( k_watertight_pair, UNIT_GRID ( n ), 0, 0, n, o, d, quads, hit, depth );
    return hipGetLastError();
}

__global__ void k_mt ( int n, const float* o, const float* d, const float* tris, int* hit, float* out4 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    float t = 0.f; V3 p = v3 ( 0, 0, 0 );
    bool ok = moller_trumbore ( v3p ( o + 3 * i ), v3p ( d + 3 * i ), v3p ( tris + 9 * i ), v3p ( tris + 9 * i + 3 ), v3p ( tris + 9 * i + 6 ), t, p );
    hit[i] = ok ? 1 : 0;
    out4[4 * i] = ok ? t : 0.f; out4[4 * i + 1] = ok ? p.x : 0.f; out4[4 * i + 2] = ok ? p.y : 0.f; out4[4 * i + 3] = ok ? p.z : 0.f;
}
hipError_t terra_unit_moller_trumbore ( int n, const float* o, const float* d, const float* tris, int* hit, float* out4 ) {
    hipLaunchKernelGGL ( k_mt, UNIT_GRID ( n ), 0, 0, n, o, d, tris, hit, out4 );
    return hipGetLastError();
}

// unit kernels read the scene from global memory (MODE 0); LDS only holds stack + leaf list
__device__ __forceinline__ Tracer unit_tracer ( const DevScene& sc, int* lds ) {
    return unstaged_tracer ( sc, lds, ( uint32_t ) ( sc.max_stack < 1 ? 1 : sc.max_stack ), TERRA_LEAF_CAP_MAX, nullptr, 0 );      // no cull at unit level: the reference's traversal decision by decision       // (unit kernels are not built with TERRA_CHECK_BOUNDS)
}
__global__ __launch_bounds__ ( 256 ) void k_bvh_traverse ( DevScene sc, int n, const float* o, const float* d, int* found, uint32_t* prim, float* point ) {
    extern __shared__ int lds_stack[];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    Ray r = make_ray ( v3p ( o + 3 * i ), v3p ( d + 3 * i ) );
    RayState s = ray_state_init ( r );
    Counters c = counters_zero();
    Tracer T = unit_tracer ( sc, lds_stack );
    Closest b = bvh_traverse<0, 0> ( T, r, s, c );
    bool f = b.tri != 0xffffffffu;
    found[i] = f ? 1 : 0;
    prim[i] = f ? ( sc.tris[b.tri].object | ( sc.tris[b.tri].tri_in_object << 8 ) ) : 0u;
    V3 pt = f ? r.o + r.d * b.depth : v3 ( FLT_MAX, FLT_MAX, FLT_MAX );
    point[3 * i] = pt.x; point[3 * i + 1] = pt.y; point[3 * i + 2] = pt.z;
}
static size_t stack_lds ( const DevScene& sc ) { return ( size_t ) ( ( sc.max_stack < 1 ? 1 : sc.max_stack ) + TERRA_LEAF_CAP_MAX ) * 256 * sizeof ( int ); }
hipError_t terra_unit_bvh_traverse ( const DevScene& sc, int n, const float* o, const float* d, int* found, uint32_t* prim, float* point ) {
    hipLaunchKernelGGL ( k_bvh_traverse, UNIT_GRID ( n ), stack_lds ( sc ), 0, sc, n, o, d, found, prim, point );
    return hipGetLastError();
}

// the fast tree's traversal (MODE 2) ray by ray, with the nodes each ray visited: same answers as k_bvh_traverse on any ray, axis-parallel ones included
#define UNIT_FAST_STACK_LDS 32      // entries of the unit kernel's stack in LDS (32 KB per block); a deeper tree spills to `spill` like the render kernels' stacks do
__global__ __launch_bounds__ ( 256 ) void k_bvh_traverse_fast ( DevScene sc, int n, const float* o, const float* d, int* found, uint32_t* prim, float* point, uint32_t* nodes_visited, uint32_t* spill, uint32_t spill_cap, uint32_t lds_entries ) {
    extern __shared__ int lds_stack[];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    Ray r = make_ray ( v3p ( o + 3 * i ), v3p ( d + 3 * i ) );
    RayState s = ray_state_init ( r );
    Counters c = counters_zero();
    Tracer T = unstaged_tracer ( sc, lds_stack, lds_entries, 0, nullptr, 0 );
    T.spill = spill ? spill + ( size_t ) i * spill_cap : nullptr; T.spill_cap = spill_cap;          // (one lane per ray: the lane's part of the spill area is its ray's)
    ClosestRanked b = bvh_traverse_fast<1> ( T, r, s, c );
    bool f = b.tri != 0xffffffffu;
    found[i] = f ? 1 : 0;
    prim[i] = f ? ( sc.fast_tris[b.tri].object | ( sc.fast_tris[b.tri].tri_in_object << 8 ) ) : 0u;
    V3 pt = f ? r.o + r.d * b.depth : v3 ( FLT_MAX, FLT_MAX, FLT_MAX );
    point[3 * i] = pt.x; point[3 * i + 1] = pt.y; point[3 * i + 2] = pt.z;
    nodes_visited[i] = c.nodes;
}
hipError_t terra_unit_bvh_traverse_fast ( const DevScene& sc, int n, const float* o, const float* d, int* found, uint32_t* prim, float* point, uint32_t* nodes_visited ) {
    const uint32_t need = ( uint32_t ) ( sc.fast_max_stack < 1 ? 1 : sc.fast_max_stack ), lds_entries = need < UNIT_FAST_STACK_LDS ? need : UNIT_FAST_STACK_LDS, spill_cap = need - lds_entries;
    uint32_t* spill = nullptr;
    if ( spill_cap ) { const hipError_t e = hipMalloc ( ( void** ) &spill, ( size_t ) ( ( n + 255 ) / 256 ) * 256 * spill_cap * sizeof ( uint32_t ) ); if ( e != hipSuccess ) return e; }
    hipLaunchKernelGGL ( k_bvh_traverse_fast, UNIT_GRID ( n ), ( size_t ) lds_entries * 256 * sizeof ( int ), 0, sc, n, o, d, found, prim, point, nodes_visited, spill, spill_cap, lds_entries );
    hipError_t e = hipGetLastError();
    if ( spill ) { const hipError_t e2 = hipDeviceSynchronize(); if ( e == hipSuccess ) e = e2; ( void ) hipFree ( spill ); }
    return e;
}

__device__ void surface_to_floats ( const DevScene& sc, const Surface& sf, uint32_t object, float* q ) {
    Basis bs = make_basis ( sf.normal );
    q[0] = bs.r0[0]; q[1] = bs.r0[1]; q[2] = bs.r0[2]; q[3] = 0.f;
    q[4] = bs.r1[0]; q[5] = bs.r1[1]; q[6] = bs.r1[2]; q[7] = 0.f;
    q[8] = bs.r2[0]; q[9] = bs.r2[1]; q[10] = bs.r2[2]; q[11] = 0.f;
    q[12] = 0.f; q[13] = 0.f; q[14] = 0.f; q[15] = 1.f;
    q[16] = sf.normal.x; q[17] = sf.normal.y; q[18] = sf.normal.z;
    q[19] = sf.emissive.x; q[20] = sf.emissive.y; q[21] = sf.emissive.z;
    q[22] = sc.mats[object].ior;
    // the attributes as the surface carries them (a textured slot: its sample at the hit's texcoord); slots the surface does not hold: the material's constants.
    // For a surface as surface_init left it: BSDF sampling overwrites Phong slot 3 and glass slots 2, 3 (scratch), so a record taken after a sample is not this
    for ( int a = 0; a < 8; ++a ) for ( int k = 0; k < 3; ++k ) q[23 + 3 * a + k] = a < 4 ? pick ( sf.attr[a], k ) : sc.mats[object].attributes[a][k];
}
__global__ __launch_bounds__ ( 256 ) void k_raycast ( DevScene sc, int n, const float* o, const float* d, int* obj, int* tri, float* point, float* surface47 ) {
    extern __shared__ int lds_stack[];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    Ray r = make_ray ( v3p ( o + 3 * i ), v3p ( d + 3 * i ) );
    Counters c = counters_zero();
    Surface sf;
    Tracer T = unit_tracer ( sc, lds_stack );
    RaycastResult h = scene_raycast<0, 0, TERRA_KINDS_ALL> ( T, r, sf, c );
    obj[i] = h.hit ? ( int ) h.object : -1;
    tri[i] = h.hit ? ( int ) h.tri_in_object : 0;
    point[3 * i] = h.point.x; point[3 * i + 1] = h.point.y; point[3 * i + 2] = h.point.z;
    float* q = surface47 + 47 * ( size_t ) i;
    if ( h.hit ) surface_to_floats ( sc, sf, h.object, q );
    else for ( int j = 0; j < 47; ++j ) q[j] = 0.f;
}
hipError_t terra_unit_raycast ( const DevScene& sc, int n, const float* o, const float* d, int* obj, int* tri, float* point, float* surface47 ) {
    hipLaunchKernelGGL ( k_raycast, UNIT_GRID ( n ), stack_lds ( sc ), 0, sc, n, o, d, obj, tri, point, surface47 );
    return hipGetLastError();
}

template <int I>
__global__ __launch_bounds__ ( 256 ) void k_trace ( DevScene sc, uint32_t bounces, int n, const float* o, const float* d, const uint64_t* stateB, const uint64_t* incB, float* radiance, uint32_t* rand_calls ) {
    extern __shared__ int lds_stack[];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    Ray r = make_ray ( v3p ( o + 3 * i ), v3p ( d + 3 * i ) );
    Pcg32 b; b.state = stateB[i]; b.inc = incB[i];
    Counters c = counters_zero();
    Tracer T = unit_tracer ( sc, lds_stack );
    V3 L = trace_path<I, 2, 0, TERRA_KINDS_ALL> ( T, r, bounces, b, c );
    radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
    rand_calls[i] = c.rand_calls;
}
hipError_t terra_unit_trace ( const DevScene& sc, int integrator, uint32_t bounces, int n, const float* o, const float* d,
                              const uint64_t* stateB, const uint64_t* incB, float* radiance, uint32_t* rand_calls ) {
#define TRACE_CASE(I) case I: hipLaunchKernelGGL ( k_trace<I>, UNIT_GRID ( n ), stack_lds ( sc ), 0, sc, bounces, n, o, d, stateB, incB, radiance, rand_calls ); break;
    switch ( integrator ) {
        TRACE_CASE ( 0 ) TRACE_CASE ( 1 ) TRACE_CASE ( 2 ) TRACE_CASE ( 3 ) TRACE_CASE ( 4 ) TRACE_CASE ( 5 ) TRACE_CASE ( 6 )
        default: return hipErrorInvalidValue;
    }
#undef TRACE_CASE
    return hipGetLastError();
}

__global__ void k_bsdf ( int kind, int n, float* surfaces47, const float* e3, const float* wo3, float* wi3, float* pdf, float* f3 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    float* q = surfaces47 + 47 * ( size_t ) i;
    Surface sf;
    // the tangent frame is a function of the normal (terra_f4x4_basis); q[0..15] is not read
    sf.normal = v3p ( q + 16 ); sf.emissive = v3p ( q + 19 );
    for ( int a = 0; a < 4; ++a ) sf.attr[a] = v3p ( q + 23 + 3 * a );
    sf.bsdf = kind; sf.ior = q[22];
    V3 wo = v3p ( wo3 + 3 * i );
    V3 wi = bsdf_sample<TERRA_KINDS_ALL> ( sf, e3[3 * i], e3[3 * i + 1], e3[3 * i + 2], wo, azimuth_fetch ( nullptr, e3[3 * i + 1] ) );          // (a stream-B value computes from its 24 bits, as a render does; any other float by tdm_sincosf_pair)
    float p = bsdf_pdf<TERRA_KINDS_ALL> ( sf, wi, wo );
    V3 f = bsdf_eval<TERRA_KINDS_ALL> ( sf, wi, wo );
    wi3[3 * i] = wi.x; wi3[3 * i + 1] = wi.y; wi3[3 * i + 2] = wi.z;
    pdf[i] = p;
    f3[3 * i] = f.x; f3[3 * i + 1] = f.y; f3[3 * i + 2] = f.z;
    q[23 + 6] = sf.attr[2].x; q[23 + 7] = sf.attr[2].y; q[23 + 8] = sf.attr[2].z; q[23 + 9] = sf.attr[3].x;
}
hipError_t terra_unit_bsdf ( int kind, int n, float* surfaces47, const float* e3, const float* wo3, float* wi3, float* pdf, float* f3 ) {
    hipLaunchKernelGGL ( k_bsdf, UNIT_GRID ( n ), 0, 0, kind, n, surfaces47, e3, wo3, wi3, pdf, f3 );
    return hipGetLastError();
}

// pdf and eval at a GIVEN pair of directions, no sample first (what Direct and Direct + MIS do at a light's direction). The surfaces are read only:
// Phong reads its slot 3 and glass its slots 2, 3 (the scratch a sample left) as handed in
__global__ void k_bsdf_at ( int kind, int n, const float* surfaces47, const float* wi3, const float* wo3, float* pdf, float* f3 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    const float* q = surfaces47 + 47 * ( size_t ) i;
    Surface sf;
    sf.normal = v3p ( q + 16 ); sf.emissive = v3p ( q + 19 );
    for ( int a = 0; a < 4; ++a ) sf.attr[a] = v3p ( q + 23 + 3 * a );
    sf.bsdf = kind; sf.ior = q[22];
    V3 wi = v3p ( wi3 + 3 * i ), wo = v3p ( wo3 + 3 * i );
    float p = bsdf_pdf<TERRA_KINDS_ALL> ( sf, wi, wo );
    V3 f = bsdf_eval<TERRA_KINDS_ALL> ( sf, wi, wo );
    pdf[i] = p;
    f3[3 * i] = f.x; f3[3 * i + 1] = f.y; f3[3 * i + 2] = f.z;
}
hipError_t terra_unit_bsdf_at ( int kind, int n, const float* surfaces47, const float* wi3, const float* wo3, float* pdf, float* f3 ) {
    hipLaunchKernelGGL ( k_bsdf_at, UNIT_GRID ( n ), 0, 0, kind, n, surfaces47, wi3, wo3, pdf, f3 );
    return hipGetLastError();
}

__global__ void k_camera ( DevRenderParams p, int n, const uint32_t* xy2, const float* r2, float* dirs3 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    V3 d = camera_sample ( p, xy2[2 * i], xy2[2 * i + 1], r2[2 * i], r2[2 * i + 1] );
    dirs3[3 * i] = d.x; dirs3[3 * i + 1] = d.y; dirs3[3 * i + 2] = d.z;
}
hipError_t terra_unit_camera ( const DevRenderParams& p, int n, const uint32_t* xy2, const float* r2, float* dirs3 ) {
    hipLaunchKernelGGL ( k_camera, UNIT_GRID ( n ), 0, 0, p, n, xy2, r2, dirs3 );
    return hipGetLastError();
}

__global__ void k_tonemap ( int op, float gamma, int n, float* c3 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    V3 c = tonemap ( v3p ( c3 + 3 * i ), op, gamma );
    c3[3 * i] = c.x; c3[3 * i + 1] = c.y; c3[3 * i + 2] = c.z;
}
hipError_t terra_unit_tonemap ( int op, float gamma, int n, float* colors3 ) {
    hipLaunchKernelGGL ( k_tonemap, UNIT_GRID ( n ), 0, 0, op, gamma, n, colors3 );
    return hipGetLastError();
}

__global__ void k_math ( int fn, int n, const float* x, const float* y, float* out ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    float r;
    switch ( fn ) {
        case 0: r = tdm_sinf ( x[i] ); break;
        case 1: r = tdm_cosf ( x[i] ); break;
        case 2: r = tdm_powf ( x[i], y[i] ); break;
        case 3: r = tdm_acosf ( x[i] ); break;
        default: r = tdm_atan2f ( x[i], y[i] ); break;
    }
    out[i] = r;
}
hipError_t terra_unit_math ( int fn, int n, const float* x, const float* y, float* out ) {
    hipLaunchKernelGGL ( k_math, UNIT_GRID ( n ), 0, 0, fn, n, x, y, out );
    return hipGetLastError();
}

// ---- exact_div.h against the plain "/" (tests/test_exact_div_gpu.py). Per element both are computed and their bits compared ON THE DEVICE (NaN = NaN): *mismatches counts
// the elements that differ and first_bad keeps the first 16 of them as {inputs[3], helper bits[3], plain bits[3]}. Two forms: explicit -- elements read from a / b / c,
// both results also stored, so the caller can compare them itself -- and generated (a == nullptr) -- element k of the set made from the counter, for the sets that are too
// large to store: every bit pattern (ops 0, 1), hashed pairs (2), pairs built around rounding midpoints and representable quotients (3), hashed vectors (4).
//   op 0  rcp_exact ( d )                                   generated: d = the pattern k
//   op 1  div_exact_rk ( x, D, R ), D / R launch constants   generated: x = the pattern k
//   op 2  div_exact_r ( x, d, rcp_exact ( d ) )              generated: even k: two patterns uniform in bits; odd k: both inside the guarded range
//   op 3  the same on generated pairs only: d and a target quotient q hashed from k, x = RN ( d (q + s ulp(q) / 2) ), s = -1, 0, +1 by k, and x's two float neighbours
//   op 4  normalize ( x, y, z ) against normalize_plain       generated: three components hashed from k (every fourth vector uniform in bits)
struct XdSink { unsigned long long* mismatches; uint32_t* first_bad; };
TD uint64_t xd_hash ( uint64_t x ) { x += 0x9e3779b97f4a7c15ull; x = ( x ^ ( x >> 30 ) ) * 0xbf58476d1ce4e5b9ull; x = ( x ^ ( x >> 27 ) ) * 0x94d049bb133111ebull; return x ^ ( x >> 31 ); }
// a float of random sign and significand with its exponent field in [lo, lo + span)
TD float xd_float_in ( uint32_t h, uint32_t lo, uint32_t span ) { return __uint_as_float ( ( h & 0x807fffffu ) | ( ( lo + ( ( h >> 23 ) & 0xffu ) % span ) << 23 ) ); }
TD bool xd_same ( float h, float p ) { return __float_as_uint ( h ) == __float_as_uint ( p ) || ( h != h && p != p ); }
TD void xd_check ( const XdSink& s, V3 in, V3 h, V3 p ) {
    if ( xd_same ( h.x, p.x ) && xd_same ( h.y, p.y ) && xd_same ( h.z, p.z ) ) return;
    const unsigned long long slot = atomicAdd ( s.mismatches, 1ull );
    if ( slot < 16ull ) {
        uint32_t* r = s.first_bad + 9 * slot;
        r[0] = __float_as_uint ( in.x ); r[1] = __float_as_uint ( in.y ); r[2] = __float_as_uint ( in.z );
        r[3] = __float_as_uint ( h.x ); r[4] = __float_as_uint ( h.y ); r[5] = __float_as_uint ( h.z );
        r[6] = __float_as_uint ( p.x ); r[7] = __float_as_uint ( p.y ); r[8] = __float_as_uint ( p.z );
    }
}
TD void xd_pair ( const XdSink& s, float x, float d ) { xd_check ( s, v3 ( x, d, 0.f ), v3 ( div_exact_r ( x, d, rcp_exact ( d ) ), 0.f, 0.f ), v3 ( x / d, 0.f, 0.f ) ); }
template <int OP>
__global__ __launch_bounds__ ( 256 ) void k_exact_div ( const float* a, const float* b, const float* c, unsigned long long first, unsigned long long count, float D, float R, unsigned long long seed,
                                                        uint32_t* helper_bits, uint32_t* plain_bits, XdSink s ) {
    const unsigned long long stride = ( unsigned long long ) gridDim.x * blockDim.x;
    for ( unsigned long long i = ( unsigned long long ) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride ) {
        const unsigned long long k = first + i;
        const uint64_t h0 = xd_hash ( seed ^ ( k * 0xd1342543de82ef95ull ) ), h1 = xd_hash ( h0 );
        if ( OP == 3 ) {
            const float d = xd_float_in ( ( uint32_t ) h0, 107u, 40u ), q = xd_float_in ( ( uint32_t ) ( h0 >> 32 ), 107u, 40u );
            const double half_ulp = ( double ) __uint_as_float ( ( __float_as_uint ( q ) & 0x7f800000u ) - ( 24u << 23 ) );          // 2^(e - 24): half a unit of q's last place
            const double target = ( double ) q + ( double ) ( ( int ) ( k % 3ull ) - 1 ) * half_ulp;
            const float x = ( float ) ( ( double ) d * target );          // (24 x 25 bits: the product is exact, the conversion rounds to nearest)
            xd_pair ( s, x, d );
            xd_pair ( s, __uint_as_float ( __float_as_uint ( x ) + 1u ), d );
            xd_pair ( s, __uint_as_float ( __float_as_uint ( x ) - 1u ), d );
            continue;
        }
        V3 in = v3 ( 0.f, 0.f, 0.f ), hv = in, pv = in;
        if ( a ) { in.x = a[i]; if ( OP == 2 || OP == 4 ) in.y = b[i]; if ( OP == 4 ) in.z = c[i]; }
        else if ( OP == 0 || OP == 1 ) in.x = __uint_as_float ( ( uint32_t ) k );
        else if ( OP == 2 ) {
            if ( k & 1ull ) { in.x = xd_float_in ( ( uint32_t ) h0, 67u, 121u ); in.y = xd_float_in ( ( uint32_t ) ( h0 >> 32 ), 67u, 121u ); }
            else { in.x = __uint_as_float ( ( uint32_t ) h0 ); in.y = __uint_as_float ( ( uint32_t ) ( h0 >> 32 ) ); }
        } else {
            if ( ( k & 3ull ) == 3ull ) in = v3 ( __uint_as_float ( ( uint32_t ) h0 ), __uint_as_float ( ( uint32_t ) ( h0 >> 32 ) ), __uint_as_float ( ( uint32_t ) h1 ) );
            else { const uint32_t lo = 87u + ( uint32_t ) ( h1 >> 40 ) % 60u; in = v3 ( xd_float_in ( ( uint32_t ) h0, lo, 24u ), xd_float_in ( ( uint32_t ) ( h0 >> 32 ), lo, 24u ), xd_float_in ( ( uint32_t ) h1, lo, 24u ) ); }
        }
        if ( OP == 0 ) { hv.x = rcp_exact ( in.x ); pv.x = 1.f / in.x; }
        else if ( OP == 1 ) { hv.x = div_exact_rk ( in.x, D, R ); pv.x = in.x / D; }
        else if ( OP == 2 ) { hv.x = div_exact_r ( in.x, in.y, rcp_exact ( in.y ) ); pv.x = in.x / in.y; }
        else { hv = normalize ( in ); pv = normalize_plain ( in ); }
        xd_check ( s, in, hv, pv );
        if ( a ) {
            if ( OP == 4 ) { helper_bits[3 * i] = __float_as_uint ( hv.x ); helper_bits[3 * i + 1] = __float_as_uint ( hv.y ); helper_bits[3 * i + 2] = __float_as_uint ( hv.z );
                             plain_bits[3 * i] = __float_as_uint ( pv.x ); plain_bits[3 * i + 1] = __float_as_uint ( pv.y ); plain_bits[3 * i + 2] = __float_as_uint ( pv.z ); }
            else { helper_bits[i] = __float_as_uint ( hv.x ); plain_bits[i] = __float_as_uint ( pv.x ); }
        }
    }
}
hipError_t terra_unit_exact_div ( int op, const float* a, const float* b, const float* c, uint64_t first, uint64_t count, float D, float R, uint64_t seed,
                                  uint32_t* helper_bits, uint32_t* plain_bits, unsigned long long* mismatches, uint32_t* first_bad ) {
    if ( count == 0 ) return hipSuccess;
    const uint64_t blocks = ( count + 255u ) / 256u;
    const dim3 grid ( ( unsigned ) ( blocks < 4096u ? blocks : 4096u ) ), block ( 256 );          // (grid-stride: a set of 2^32 elements is 4096 trips of a lane)
    const XdSink s = { mismatches, first_bad };
#define XD_CASE(OP) case OP: hipLaunchKernelGGL ( k_exact_div<OP>, grid, block, 0, 0, a, b, c, ( unsigned long long ) first, ( unsigned long long ) count, D, R, ( unsigned long long ) seed, helper_bits, plain_bits, s ); break;
    switch ( op ) {
        XD_CASE ( 0 ) XD_CASE ( 1 ) XD_CASE ( 2 ) XD_CASE ( 3 ) XD_CASE ( 4 )
        default: return hipErrorInvalidValue;
    }
#undef XD_CASE
    return hipGetLastError();
}

// ---- exact_sqrt.h, the one-path make_basis and roulette_scale against their plain forms (tests/test_exact_sqrt_gpu.py), in the manner of k_exact_div: both computed per
// element, bits compared on the device (NaN = NaN), *mismatches and the first 16 offenders as {inputs[3], helper bits[9], plain bits[9]} (unused words 0). Explicit form:
// elements read from a / b / c, both results also stored, `per` words per element; generated form (a == nullptr): element k of a set made from the counter.
//   op 0  sqrt_exact ( x ) against sqrtf ( x )                       per 1   generated: x = the pattern k
//   op 1  a deliberately wrong core (the upper candidate dropped) against sqrtf: the comparison's positive control          generated: x = the pattern k
//   op 2  make_basis ( n ) against make_basis_plain ( n )            per 9   generated: n a hashed unit vector, scaled by 1, 2^40 or 2^-40 by k; every fourth uniform in bits
//   op 3  roulette_scale ( pr ) against the plain expression         per 1   generated: pr = the pattern k
//   op 4  normalize ( x, y, z ) against normalize_plain              per 3   generated: k_exact_div's vectors; every eighth with components of magnitude 2^-49 .. 2^-47 or
//                                                                            2^47 .. 2^49, so that the squared length falls on either side of the root's guard 2^-96 (and of 2^96)
struct XsSink { unsigned long long* mismatches; uint32_t* first_bad; };
TD float xs_sqrt_wrong ( float x ) {
    if ( !xs_in_range ( x ) ) return sqrtf ( x );
    const float s = __builtin_amdgcn_sqrtf ( x );
    const float down = __uint_as_float ( __float_as_uint ( s ) - 1u );
    return __builtin_fmaf ( -down, s, x ) <= 0.f ? down : s;
}
TD void basis_words ( const Basis& m, float* w ) { for ( int j = 0; j < 3; ++j ) { w[j] = m.r0[j]; w[3 + j] = m.r1[j]; w[6 + j] = m.r2[j]; } }
template <int OP>
__global__ __launch_bounds__ ( 256 ) void k_exact_sqrt ( const float* a, const float* b, const float* c, unsigned long long first, unsigned long long count, unsigned long long seed,
                                                         uint32_t* helper_bits, uint32_t* plain_bits, XsSink s ) {
    constexpr int PER = OP == 2 ? 9 : ( OP == 4 ? 3 : 1 );
    const unsigned long long stride = ( unsigned long long ) gridDim.x * blockDim.x;
    for ( unsigned long long i = ( unsigned long long ) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride ) {
        const unsigned long long k = first + i;
        const uint64_t h0 = xd_hash ( seed ^ ( k * 0xd1342543de82ef95ull ) ), h1 = xd_hash ( h0 );
        V3 in = v3 ( 0.f, 0.f, 0.f );
        if ( a ) { in.x = a[i]; if ( OP == 2 || OP == 4 ) { in.y = b[i]; in.z = c[i]; } }
        else if ( OP == 0 || OP == 1 || OP == 3 ) in.x = __uint_as_float ( ( uint32_t ) k );
        else if ( ( k & 3ull ) == 3ull ) in = v3 ( __uint_as_float ( ( uint32_t ) h0 ), __uint_as_float ( ( uint32_t ) ( h0 >> 32 ) ), __uint_as_float ( ( uint32_t ) h1 ) );
        else if ( OP == 2 ) {
            in = normalize_plain ( v3 ( xd_float_in ( ( uint32_t ) h0, 115u, 13u ), xd_float_in ( ( uint32_t ) ( h0 >> 32 ), 115u, 13u ), xd_float_in ( ( uint32_t ) h1, 115u, 13u ) ) );
            const uint32_t pick3 = ( uint32_t ) ( h1 >> 40 ) % 3u;
            in = in * ( pick3 == 0u ? 1.f : ( pick3 == 1u ? 0x1p40f : 0x1p-40f ) );
        } else if ( ( k & 7ull ) == 5ull ) {
            const uint32_t lo = ( h1 >> 40 ) & 1u ? 78u : 174u;
            in = v3 ( xd_float_in ( ( uint32_t ) h0, lo, 3u ), xd_float_in ( ( uint32_t ) ( h0 >> 32 ), lo, 3u ), xd_float_in ( ( uint32_t ) h1, lo, 3u ) );
        } else {
            const uint32_t lo = 87u + ( uint32_t ) ( h1 >> 40 ) % 60u;
            in = v3 ( xd_float_in ( ( uint32_t ) h0, lo, 24u ), xd_float_in ( ( uint32_t ) ( h0 >> 32 ), lo, 24u ), xd_float_in ( ( uint32_t ) h1, lo, 24u ) );
        }
        float hw[9] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f }, pw[9] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
        if ( OP == 0 ) { hw[0] = sqrt_exact ( in.x ); pw[0] = sqrtf ( in.x ); }
        else if ( OP == 1 ) { hw[0] = xs_sqrt_wrong ( in.x ); pw[0] = sqrtf ( in.x ); }
        else if ( OP == 2 ) { basis_words ( make_basis ( in ), hw ); basis_words ( make_basis_plain ( in ), pw ); }
        else if ( OP == 3 ) { hw[0] = roulette_scale ( in.x ); pw[0] = ( float ) ( 1.0 / ( ( double ) in.x + 1e-4 ) ); }
        else { const V3 hv = normalize ( in ), pv = normalize_plain ( in ); hw[0] = hv.x; hw[1] = hv.y; hw[2] = hv.z; pw[0] = pv.x; pw[1] = pv.y; pw[2] = pv.z; }
        bool same = true;
        for ( int j = 0; j < PER; ++j ) same = same && xd_same ( hw[j], pw[j] );
        if ( !same ) {
            const unsigned long long slot = atomicAdd ( s.mismatches, 1ull );
            if ( slot < 16ull ) {
                uint32_t* r = s.first_bad + 21 * slot;
                r[0] = __float_as_uint ( in.x ); r[1] = __float_as_uint ( in.y ); r[2] = __float_as_uint ( in.z );
                for ( int j = 0; j < 9; ++j ) { r[3 + j] = __float_as_uint ( hw[j] ); r[12 + j] = __float_as_uint ( pw[j] ); }
            }
        }
        if ( a ) for ( int j = 0; j < PER; ++j ) { helper_bits[PER * i + j] = __float_as_uint ( hw[j] ); plain_bits[PER * i + j] = __float_as_uint ( pw[j] ); }
    }
}
hipError_t terra_unit_exact_sqrt ( int op, const float* a, const float* b, const float* c, uint64_t first, uint64_t count, uint64_t seed,
                                   uint32_t* helper_bits, uint32_t* plain_bits, unsigned long long* mismatches, uint32_t* first_bad ) {
    if ( count == 0 ) return hipSuccess;
    const uint64_t blocks = ( count + 255u ) / 256u;
    const dim3 grid ( ( unsigned ) ( blocks < 4096u ? blocks : 4096u ) ), block ( 256 );
    const XsSink s = { mismatches, first_bad };
#define XS_CASE(OP) case OP: hipLaunchKernelGGL ( k_exact_sqrt<OP>, grid, block, 0, 0, a, b, c, ( unsigned long long ) first, ( unsigned long long ) count, ( unsigned long long ) seed, helper_bits, plain_bits, s ); break;
    switch ( op ) {
        XS_CASE ( 0 ) XS_CASE ( 1 ) XS_CASE ( 2 ) XS_CASE ( 3 ) XS_CASE ( 4 )
        default: return hipErrorInvalidValue;
    }
#undef XS_CASE
    return hipGetLastError();
}

// ---- the texture lookups on one texture of a blob (scene_host.cpp unit_texture): texture_sample in texel units, and environment_eval by direction on a scene
// record that holds nothing but that texture as its lat-long environment
__global__ void k_texture_sample ( const DevTexture* t, int n, const float* uv2, float* out3 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    V3 c = texture_sample ( *t, uv2[2 * i], uv2[2 * i + 1] );
    out3[3 * i] = c.x; out3[3 * i + 1] = c.y; out3[3 * i + 2] = c.z;
}
hipError_t terra_unit_texture_sample ( const DevTexture* t, int n, const float* uv2, float* out3 ) {
    if ( n > 0 ) hipLaunchKernelGGL ( k_texture_sample, UNIT_GRID ( n ), 0, 0, t, n, uv2, out3 );
    return hipGetLastError();
}
__global__ void k_texture_latlong ( DevScene sc, int n, const float* dir3, float* out3 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    V3 c = environment_eval ( sc, v3p ( dir3 + 3 * i ) );
    out3[3 * i] = c.x; out3[3 * i + 1] = c.y; out3[3 * i + 2] = c.z;
}
hipError_t terra_unit_texture_latlong ( const DevTexture* t, int n, const float* dir3, float* out3 ) {
    DevScene sc {};
    sc.textures = t; sc.env_mode = 2; sc.env_tex = 0;
    if ( n > 0 ) hipLaunchKernelGGL ( k_texture_latlong, UNIT_GRID ( n ), 0, 0, sc, n, dir3, out3 );
    return hipGetLastError();
}

// ---- SURVEY.md 8f N4, unit level: samplers and distributions (sampling_device.h) ---------------------------------------------
// one sampler per seed; a stratified sampler's n pairs are inherently sequential (they share one random stream)
__global__ void k_stratified ( const uint32_t* seeds, int nseeds, int strata, int samples, int n, float* out2 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= nseeds ) return;
    StratifiedSampler s; stratified_init ( s, seeds[i], strata, samples );
    for ( int j = 0; j < n; ++j ) { float a, b; stratified_next_pair ( s, a, b ); out2[ ( ( size_t ) i * n + j ) * 2] = a; out2[ ( ( size_t ) i * n + j ) * 2 + 1] = b; }
}
hipError_t terra_unit_stratified ( const uint32_t* seeds, int nseeds, int strata, int samples, int n, float* out2 ) {
    hipLaunchKernelGGL ( k_stratified, UNIT_GRID ( nseeds ), 0, 0, seeds, nseeds, strata, samples, n, out2 );
    return hipGetLastError();
}
__global__ void k_halton ( int first, int n, float* out2 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    float a, b; halton_pair ( first + i, a, b );
    out2[2 * i] = a; out2[2 * i + 1] = b;
}
hipError_t terra_unit_halton ( int first, int n, float* out2 ) {
    hipLaunchKernelGGL ( k_halton, UNIT_GRID ( n ), 0, 0, first, n, out2 );
    return hipGetLastError();
}
// rows of a 2D table (ny = 1: a 1D distribution): one lane per row, each a sequential float sum
__global__ void k_dist_rows ( const float* f, uint32_t nx, uint32_t ny, float* cdf, float* integrals, uint32_t* monotone ) {
    uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if ( r >= ny ) return;
    integrals[r] = distribution_row_init ( f + ( size_t ) nx * r, nx, cdf + ( size_t ) nx * r, monotone + r );
}
// the marginal over the rows' totals (reference src/Terra.c:817-833): one lane, sequential; slot ny of `integrals` / `monotone` receives its total / flag
__global__ void k_dist_marginal ( uint32_t ny, float* integrals, float* mcdf, uint32_t* monotone ) {
    if ( blockIdx.x || threadIdx.x ) return;
    integrals[ny] = distribution_row_init ( integrals, ny, mcdf, monotone + ny );
}
__global__ void k_dist_sample_1d ( const float* f, const float* cdf, uint32_t n, const float* integral, const uint32_t* monotone, const float* e, int m, float* x, float* pdf, uint32_t* idx ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= m ) return;
    DevDistribution1D d = { f, cdf, n, integral[0], monotone[0] };
    float p = 0.f; uint32_t k = 0;
    x[i] = distribution_sample ( d, e[i], &p, &k );
    pdf[i] = p; idx[i] = k;
}
__global__ void k_dist_sample_2d ( const float* f, const float* cdf, uint32_t nx, uint32_t ny, const float* integrals, const float* mcdf, const uint32_t* monotone, const float* e12, int m, float* xy2, float* pdf ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= m ) return;
    DevDistribution1D marginal = { integrals, mcdf, ny, integrals[ny], monotone[ny] };
    float p0 = 0.f, p1 = 0.f; uint32_t row = 0;
    const float s1 = distribution_sample ( marginal, e12[2 * i], &p0, &row );
    if ( s1 == FLT_MAX ) { xy2[2 * i] = xy2[2 * i + 1] = FLT_MAX; pdf[i] = 0.f; return; }
    DevDistribution1D cond = { f + ( size_t ) nx * row, cdf + ( size_t ) nx * row, nx, integrals[row], monotone[row] };
    const float s2 = distribution_sample ( cond, e12[2 * i + 1], &p1, nullptr );
    xy2[2 * i] = s1; xy2[2 * i + 1] = s2; pdf[i] = p0 * p1;
}
hipError_t terra_unit_distribution_1d ( const float* f, uint32_t n, float* cdf, float* integral, uint32_t* monotone, const float* e, int m, float* x, float* pdf, uint32_t* idx ) {
    hipLaunchKernelGGL ( k_dist_rows, dim3 ( 1 ), dim3 ( 64 ), 0, 0, f, n, 1u, cdf, integral, monotone );
    if ( m > 0 ) hipLaunchKernelGGL ( k_dist_sample_1d, UNIT_GRID ( m ), 0, 0, f, cdf, n, integral, monotone, e, m, x, pdf, idx );
    return hipGetLastError();
}
hipError_t terra_unit_distribution_2d ( const float* f, uint32_t nx, uint32_t ny, float* cdf, float* integrals, float* mcdf, uint32_t* monotone, const float* e12, int m, float* xy2, float* pdf ) {
    hipLaunchKernelGGL ( k_dist_rows, UNIT_GRID ( ny ), 0, 0, f, nx, ny, cdf, integrals, monotone );
    hipLaunchKernelGGL ( k_dist_marginal, dim3 ( 1 ), dim3 ( 64 ), 0, 0, ny, integrals, mcdf, monotone );
    if ( m > 0 ) hipLaunchKernelGGL ( k_dist_sample_2d, UNIT_GRID ( m ), 0, 0, f, cdf, nx, ny, integrals, mcdf, monotone, e12, m, xy2, pdf );
    return hipGetLastError();
}
// the lookup environment MIS uses (integrators_device.h environment_pdf): point (v, u) of the unit square -- the order k_dist_sample_2d reports a sample in -- lies in
// bucket (row, col) = (v ny, u nx) truncated; its probability is distribution_2d_prob's (points outside [0, 1) clamp to the border buckets)
__global__ void k_dist_pdf_2d ( const float* f, uint32_t nx, uint32_t ny, const float* integrals, const float* xy2, int m, float* pdf ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= m ) return;
    const float v = xy2[2 * i], u = xy2[2 * i + 1];
    uint32_t row = v > 0.f ? ( uint32_t ) ( v * ( float ) ny ) : 0u, col = u > 0.f ? ( uint32_t ) ( u * ( float ) nx ) : 0u;
    row = row < ny - 1u ? row : ny - 1u; col = col < nx - 1u ? col : nx - 1u;
    pdf[i] = distribution_2d_prob ( f, integrals, nx, integrals[ny], row, col );
}
hipError_t terra_unit_distribution_2d_pdf ( const float* f, uint32_t nx, uint32_t ny, float* cdf, float* integrals, float* mcdf, uint32_t* monotone, const float* xy2, int m, float* pdf ) {
    hipLaunchKernelGGL ( k_dist_rows, UNIT_GRID ( ny ), 0, 0, f, nx, ny, cdf, integrals, monotone );
    hipLaunchKernelGGL ( k_dist_marginal, dim3 ( 1 ), dim3 ( 64 ), 0, 0, ny, integrals, mcdf, monotone );
    if ( m > 0 ) hipLaunchKernelGGL ( k_dist_pdf_2d, UNIT_GRID ( m ), 0, 0, f, nx, ny, integrals, xy2, m, pdf );
    return hipGetLastError();
}

// ---- DevScene::sincos24: (cos, sin) of 2 * terra_PI * (k * 2^-24) for every 24-bit k, each entry by tdm_sincosf_pair itself (shading_device.h azimuth_fetch_index) ----
__global__ __launch_bounds__ ( 256 ) void terra_sincos24_kernel ( float2* table ) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;          // grid = 2^24 / 256 blocks
    float sn, cs;
    tdm_sincosf_pair ( 2 * TERRA_PI_F * ( ( float ) k * 0x1p-24f ), sn, cs );
    table[k] = make_float2 ( cs, sn );
}
hipError_t terra_fill_sincos24 ( float2* table, hipStream_t stream ) {
    hipLaunchKernelGGL ( terra_sincos24_kernel, dim3 ( ( 1u << 24 ) / 256u ), dim3 ( 256 ), 0, stream, table );
    return hipGetLastError();
}
// tdm_azimuth24 against the table, which stays its independent witness: computed[k] = what the single-arm form gives for k, in the table's layout, and
// *mismatches counts the entries whose bits differ from table[k] (either word)
__global__ __launch_bounds__ ( 256 ) void k_azimuth24 ( const float2* table, float2* computed, uint32_t* mismatches ) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;          // grid = 2^24 / 256 blocks
    float sn, cs;
    tdm_azimuth24 ( k, sn, cs );
    computed[k] = make_float2 ( cs, sn );
    const float2 t = table[k];
    if ( __float_as_uint ( t.x ) != __float_as_uint ( cs ) || __float_as_uint ( t.y ) != __float_as_uint ( sn ) ) atomicAdd ( mismatches, 1u );
}
hipError_t terra_unit_azimuth24 ( const float2* table, float2* computed, uint32_t* mismatches ) {
    hipLaunchKernelGGL ( k_azimuth24, dim3 ( ( 1u << 24 ) / 256u ), dim3 ( 256 ), 0, 0, table, computed, mismatches );
    return hipGetLastError();
}

// ---- the shading stages (exact_div.h "Shading stages") against the guarded code they stand in for (tests/test_shade_stages_gpu.py). One row of 16 floats per thread;
// per row the stage as the render loop runs it -- the short sequences unguarded, one vote over the wave, the guarded code for the whole wave where a lane failed --
// then the guarded code alone, and the stage's lane mask. 64 consecutive rows share a wave and a vote. Eight result words per row and form (unused ones 0):
//   stage 1  ray_stage:       row = d[3]                                                    words = inv[3]                 guarded = make_ray_guarded
//   stage 2  surface_stage:   row = nu, nv, div, na[3], nb[3], nc[3]                       words = u, v, normal[3]        guarded = surface_stage<false> (surface_init's lines)
//   stage 3  continue_stage:  row = n[3], albedo[3], throughput[3], k0, k1 (words), e3     words = wi[3], t[3], go        guarded = path_continue<1> itself; its word 7: the sites' own guards, a bit each
//            (k0, k1: the 24 bits of the first two variates; the azimuth is computed from k1 as a launch without a table does)
//   stage 5  camera_film_normalize: row = fx, fy (a film vector ( fx, fy, 1 ) of a launch inside the camera limits)   words = d[3]   guarded = normalize_plain
// DROPS (stages 1 and 3): the stage without the range tests its data cannot fail (stage 1: no component of 8 or more in magnitude). full_mask: the same
// stage's mask with every range test made.
template <int STAGE, bool DROPS>
__global__ __launch_bounds__ ( 256 ) void k_shade_stages ( const float* rows, unsigned long long n, uint32_t* staged, uint32_t* guarded, uint32_t* mask, uint32_t* full_mask ) {
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    if ( i >= n ) return;
    const float* q = rows + 16 * i;
    float s[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f }, g[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    int ok = 0, full = 0;
    if constexpr ( STAGE == 1 ) {
        const V3 o = v3 ( 0, 0, 0 ), d = v3p ( q );
        Ray a, b, f; bool gd;
        ok = ray_stage<true, DROPS> ( o, d, a ); full = ray_stage<true, false> ( o, d, f );
        if ( __any ( !ok ) ) a = make_ray_guarded ( o, d, gd );
        b = make_ray_guarded ( o, d, gd );
        s[0] = a.inv.x; s[1] = a.inv.y; s[2] = a.inv.z; g[0] = b.inv.x; g[1] = b.inv.y; g[2] = b.inv.z;
    } else if constexpr ( STAGE == 5 ) {          // the film vector's normalisation without a range test (trace_geometry.h camera_film_normalize): row = fx, fy
        const V3 a = camera_film_normalize ( q[0], q[1] ), b = normalize_plain ( v3 ( q[0], q[1], 1.f ) );
        ok = 1; full = 1;
        s[0] = a.x; s[1] = a.y; s[2] = a.z; g[0] = b.x; g[1] = b.y; g[2] = b.z;
    } else if constexpr ( STAGE == 2 ) {
        const float nu = q[0], nv = q[1], div = q[2], rdiv = rcp_exact ( div ); const int flag = xd_rcp_ok ( div );          // (the constants as make_tracer stages them)
        const V3 na = v3p ( q + 3 ), nb = v3p ( q + 6 ), nc = v3p ( q + 9 );
        V3 ns, ng;
        ok = surface_stage<true> ( nu, nv, div, rdiv, flag, na, nb, nc, s[0], s[1], ns ); full = ok;
        if ( __any ( !ok ) ) surface_stage<false> ( nu, nv, div, rdiv, flag, na, nb, nc, s[0], s[1], ns );
        surface_stage<false> ( nu, nv, div, rdiv, flag, na, nb, nc, g[0], g[1], ng );
        s[2] = ns.x; s[3] = ns.y; s[4] = ns.z; g[2] = ng.x; g[3] = ng.y; g[4] = ng.z;
    } else {
        const V3 nrm = v3p ( q ), albedo = v3p ( q + 3 ), tp = v3p ( q + 6 );
        const uint32_t k0 = __float_as_uint ( q[9] ) & 0xffffffu, k1 = __float_as_uint ( q[10] ) & 0xffffffu;
        PathDraws d; d.e0 = trng_b_from_bits ( k0 ); d.e1 = trng_b_from_bits ( k1 ); d.e2 = 0.f; d.e3 = q[11]; d.az = azimuth_fetch_index ( nullptr, k1 );
        V3 ws, ts, wg, tg, wf, tf; bool gs, gg, gf;
        ok = continue_stage<true, DROPS> ( nrm, albedo, tp, d, ws, ts, gs ); full = continue_stage<true, false> ( nrm, albedo, tp, d, wf, tf, gf );
        if ( __any ( !ok ) ) continue_stage<false, false> ( nrm, albedo, tp, d, ws, ts, gs );
        // the guarded code: path_continue<1> itself, on a diffuse surface with this normal and albedo (it returns "the path lives" while the bounce limit is far)
        Surface sf; sf.normal = nrm; sf.emissive = v3 ( 0, 0, 0 ); sf.attr[0] = albedo; sf.attr[1] = sf.attr[2] = sf.attr[3] = v3 ( 0, 0, 0 ); sf.ior = 1.f; sf.bsdf = kDevBsdfDiffuse;
        uint32_t bounce = 0; tg = tp;
        gg = path_continue<1> ( sf, v3 ( 0, 0, 1 ), tg, bounce, 1000u, d, wg );
        // ... and its sites' own guards, one bit each, on the operands the plain helpers hand from site to site (diffuse_sample, make_basis, normalize, diffuse_pdf,
        // rcp_exact, roulette_scale as shading_device.h / trace_math.h / exact_div.h write them): bit 0 the root of e0, 1 the root of 1 - e0, 2 make_basis's root,
        // 3 the root of wi's squared length, 4 xd_normalize3's range tests of the length and the components, 5 its all-ones test of the length (which a stage does
        // not make: exact_div.h xd_rcp_all_ones), 6 diffuse_pdf's numerator, 7 rcp_exact ( pdf ), 8 roulette_scale's bounds where the roulette lets the path live
        {
            uint32_t bits = 0;
            const float r = sqrt_exact ( d.e0 ); float sn, cs; azimuth_sincos ( d.az, d.e1, sn, cs );
            const float om = sel_max ( 0.f, 1 - d.e0 );
            const V3 local = v3 ( r * cs, sqrt_exact ( om ), r * sn );
            const float ba = fabsf ( nrm.x ) > fabsf ( nrm.y ) ? nrm.x : nrm.y;
            const V3 v = basis_apply ( make_basis ( nrm ), local );
            const float l2 = length2 ( v ), l = sqrt_exact ( l2 );
            const V3 w = normalize ( v );
            const float num = sel_max ( 0.f, dot ( nrm, w ) ), pdf = sel_max ( diffuse_pdf ( sf, w ), ( float ) 1e-4 );
            V3 t = had ( tp, diffuse_eval ( sf ) * rcp_exact ( pdf ) ); t = t * dot ( nrm, w );
            const float pr = sel_max ( t.x, sel_max ( t.y, t.z ) );
            bits |= xs_in_range ( d.e0 ) ? 1u : 0u; bits |= xs_in_range ( om ) ? 2u : 0u; bits |= xs_in_range ( ba * ba + nrm.z * nrm.z ) ? 4u : 0u; bits |= xs_in_range ( l2 ) ? 8u : 0u;
            bits |= ( ( int ) ( l >= 0x1p-60f ) & ( int ) ( l <= 0x1p60f ) & xd_component_ok ( v.x ) & xd_component_ok ( v.y ) & xd_component_ok ( v.z ) ) ? 16u : 0u;
            bits |= ( __float_as_uint ( l ) & 0x7fffffu ) != 0x7fffffu ? 32u : 0u;
            bits |= xd_in_range ( num ) ? 64u : 0u; bits |= xd_rcp_ok ( pdf ) ? 128u : 0u;
            bits |= ( ( ( int ) ( pr >= 0.f ) & ( int ) ( pr <= 0x1p60f ) ) | ( int ) ( d.e3 > pr ) ) ? 256u : 0u;
            g[7] = __uint_as_float ( bits );
        }
        s[0] = ws.x; s[1] = ws.y; s[2] = ws.z; s[3] = ts.x; s[4] = ts.y; s[5] = ts.z; s[6] = gs ? 1.f : 0.f;
        g[0] = wg.x; g[1] = wg.y; g[2] = wg.z; g[3] = tg.x; g[4] = tg.y; g[5] = tg.z; g[6] = gg ? 1.f : 0.f;
    }
    for ( int j = 0; j < 8; ++j ) { staged[8 * i + j] = __float_as_uint ( s[j] ); guarded[8 * i + j] = __float_as_uint ( g[j] ); }
    mask[i] = ( uint32_t ) ok; full_mask[i] = ( uint32_t ) full;
}
// stage 4: the two roots of diffuse_sample on every stream-B variate e = k 2^-24 without their range tests (exact_sqrt.h xs_variate_ok) against sqrt_exact:
// *mismatches += the k whose short root of e differs from sqrt_exact ( e ) although the guard admits e, the k != 0 the guard refuses, and the k whose short root of
// sel_max ( 0, 1 - e ) differs from sqrt_exact's; and the reciprocal of a length whose significand is all ones, below
__global__ __launch_bounds__ ( 256 ) void k_variate_roots ( uint32_t* mismatches ) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;          // grid = 2^24 / 256 blocks
    const float e = trng_b_from_bits ( k ), om = sel_max ( 0.f, 1 - e );
    const bool admitted = xs_variate_ok ( e ) != 0;
    uint32_t bad = 0;
    if ( admitted && __float_as_uint ( xs_sqrt_short ( e ) ) != __float_as_uint ( sqrt_exact ( e ) ) ) ++bad;
    if ( !admitted && k != 0u ) ++bad;
    if ( __float_as_uint ( xs_sqrt_short ( om ) ) != __float_as_uint ( sqrt_exact ( om ) ) ) ++bad;
    // the closed-form reciprocal of an all-ones significand (exact_div.h xd_rcp_all_ones): every such d inside the guarded range, both signs, against 1.f / d; and a
    // numerator hashed from k over the positive ones -- at the denominator's size and up to 2^-20 of it, as a component is to its vector's length -- against "/"
    const float d = __uint_as_float ( ( ( 67u + k % 121u ) << 23 ) | 0x7fffffu | ( ( k / 121u ) & 1u ) << 31 );
    if ( k < 242u && __float_as_uint ( xd_rcp_all_ones ( d ) ) != __float_as_uint ( 1.f / d ) ) ++bad;
    const float l = __builtin_fabsf ( d );
    const uint32_t h = ( uint32_t ) xd_hash ( k );
    const float x = __uint_as_float ( ( __float_as_uint ( l ) & 0x7f800000u ) - ( ( ( h >> 23 ) % 21u ) << 23 ) | ( h & 0x807fffffu ) );
    if ( xd_in_range ( x ) && __float_as_uint ( xd_div_short_pos ( x, l, xd_rcp_short_any ( l ) ) ) != __float_as_uint ( x / l ) ) ++bad;
    if ( bad ) atomicAdd ( mismatches, bad );
}
hipError_t terra_unit_shade_stages ( int stage, int drops, const float* rows, uint64_t n, uint32_t* staged, uint32_t* guarded, uint32_t* mask, uint32_t* full_mask, uint32_t* mismatches ) {
    const dim3 grid ( ( unsigned ) ( ( n + 255 ) / 256 ) ), block ( 256 );
#define SS_CASE(S, D) hipLaunchKernelGGL ( ( k_shade_stages<S, D> ), grid, block, 0, 0, rows, ( unsigned long long ) n, staged, guarded, mask, full_mask )
    if ( stage == 4 ) hipLaunchKernelGGL ( k_variate_roots, dim3 ( ( 1u << 24 ) / 256u ), dim3 ( 256 ), 0, 0, mismatches );
    else if ( n == 0 ) return hipSuccess;
    else if ( stage == 1 ) { if ( drops ) SS_CASE ( 1, true ); else SS_CASE ( 1, false ); }
    else if ( stage == 5 ) SS_CASE ( 5, false );
    else if ( stage == 2 ) SS_CASE ( 2, false );
    else if ( stage == 3 ) { if ( drops ) SS_CASE ( 3, true ); else SS_CASE ( 3, false ); }
    else return hipErrorInvalidValue;
#undef SS_CASE
    return hipGetLastError();
}
