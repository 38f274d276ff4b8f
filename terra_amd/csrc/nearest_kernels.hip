// nearest_kernels.hip -- nearest-surface queries on a committed scene (include/terra_amd.h "Nearest-surface queries"; DESIGN.md "Nearest-surface queries"): the
// closest point of the scene to each of a client's points, read from and answered into HBM. A kernel of its own in a unit of its own: it takes no part in a render
// launch and shares no kernel with the ray queries.
//
// One lane per query, 256-lane blocks on a capped grid that strides over the queries (the grid of terra_query_kernel): a lane reads its 16-byte query as one float4
// and writes its 32-byte answer as two float4, so every access of a wave is one contiguous run. ONE device function, nearest_on_triangle, holds the rule of the
// header -- binary64, in the order written, no contraction (the unit is built with -ffp-contract=off like every other) -- and both kernels call it:
//   terra_nearest_kernel<1>  the fast tree (MODE 2 and 3 alike: a point has no reference traversal to replay). Distance ordered: per node the squared distance from P
//                            to each of the four child boxes, a conservative LOWER bound (nearest_box_bound); the lane goes on with the nearest child that can still
//                            matter and pushes the others, farthest first, on the ray traversal's stack (fast_push / fast_pop: LDS column + HBM spill, at most three
//                            pushes per node step, so terra_plan_fast_tree's depth bound holds). A child is culled only when its bound is STRICTLY greater than the
//                            best D2 so far or the limit: a triangle at exactly the best D2 may still win the tie by its smaller (object, triangle) pair.
//   terra_nearest_kernel<0>  brute force, O(n * triangles): a block stages tiles of 256 triangles of the soup in LDS and every lane tests every triangle of the tile
//                            (all lanes read the same LDS address: a broadcast). It serves the scenes without a fast tree -- small ones, for which it is the right
//                            tool, and large ones held in tree mode 0, which want terra_amd_set_tree_mode(scene, 1).
// A lane keeps (D2, object, triangle, where the triangle is) of its best candidate and evaluates the rule once more on the winner for the record: fewer live
// registers in the loops, the same bits. No atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "trace_device.h"
#include "kernels.h"
#include "launch_plan.h"

#define TERRA_NEAREST_MAX_BLOCKS_PER_CU 8
#define TERRA_NEAREST_TILE 256                // triangles of a brute-force tile: one per lane of the block, 12 KB of LDS

struct D3 { double x, y, z; };
TD D3 d3 ( double x, double y, double z ) { D3 r; r.x = x; r.y = y; r.z = z; return r; }
TD D3 widen ( float4 v ) { return d3 ( ( double ) v.x, ( double ) v.y, ( double ) v.z ); }
TD D3 dsub ( D3 a, D3 b ) { return d3 ( a.x - b.x, a.y - b.y, a.z - b.z ); }
TD D3 dadd ( D3 a, D3 b ) { return d3 ( a.x + b.x, a.y + b.y, a.z + b.z ); }
TD D3 dmul ( D3 a, double s ) { return d3 ( a.x * s, a.y * s, a.z * s ); }
TD double ddot ( D3 u, D3 v ) { return ( u.x * v.x + u.y * v.y ) + u.z * v.z; }
TD double quot0 ( double a, double b ) { return b == 0.0 ? 0.0 : a / b; }      // a quotient whose divisor is exactly 0 is taken as 0

// The rule of one triangle: Q, the feature, D2 = |P - Q|^2 (header "Closest point of one triangle": the regions in its order, the first that holds decides)
TD double nearest_on_triangle ( D3 A, D3 B, D3 C, D3 P, D3& Q, uint32_t& feature ) {
    const D3 ab = dsub ( B, A ), ac = dsub ( C, A );
    const D3 ap = dsub ( P, A ); const double d1 = ddot ( ab, ap ), d2 = ddot ( ac, ap );
    const D3 bp = dsub ( P, B ); const double d3_ = ddot ( ab, bp ), d4 = ddot ( ac, bp );
    const D3 cp = dsub ( P, C ); const double d5 = ddot ( ab, cp ), d6 = ddot ( ac, cp );
    const double vc = d1 * d4 - d3_ * d2, vb = d5 * d2 - d1 * d6, va = d3_ * d6 - d5 * d4;
    if ( d1 <= 0.0 && d2 <= 0.0 ) { Q = A; feature = 1u; }
    else if ( d3_ >= 0.0 && d4 <= d3_ ) { Q = B; feature = 2u; }
    else if ( vc <= 0.0 && d1 >= 0.0 && d3_ <= 0.0 ) { const double v = quot0 ( d1, d1 - d3_ ); Q = dadd ( A, dmul ( ab, v ) ); feature = 4u; }
    else if ( d6 >= 0.0 && d5 <= d6 ) { Q = C; feature = 3u; }
    else if ( vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 ) { const double w = quot0 ( d2, d2 - d6 ); Q = dadd ( A, dmul ( ac, w ) ); feature = 6u; }
    else if ( va <= 0.0 && ( d4 - d3_ ) >= 0.0 && ( d5 - d6 ) >= 0.0 ) { const double w = quot0 ( d4 - d3_, ( d4 - d3_ ) + ( d5 - d6 ) ); Q = dadd ( B, dmul ( dsub ( C, B ), w ) ); feature = 5u; }
    else { const double den = ( va + vb ) + vc; Q = dadd ( dadd ( A, dmul ( ab, quot0 ( vb, den ) ) ), dmul ( ac, quot0 ( vc, den ) ) ); feature = 0u; }
    const D3 e = dsub ( P, Q );
    return ddot ( e, e );
}

// a lane's best candidate: D2, the tie key, and where the triangle's three float4 are (an index into the array the kernel reads)
struct NearestBest { double d2; uint32_t object, triangle, at; };
// counts (not NaN, within the limit: r2 = +inf without one) and beats the best: smaller D2, or the same D2 with the smaller (object, triangle) pair
TD void nearest_take ( NearestBest& best, double d2, double r2, uint32_t object, uint32_t triangle, uint32_t at ) {
    if ( d2 <= r2 && ( d2 < best.d2 || ( d2 == best.d2 && ( object < best.object || ( object == best.object && triangle < best.triangle ) ) ) ) ) {      // (d2 <= r2 is false for a NaN)
        best.d2 = d2; best.object = object; best.triangle = triangle; best.at = at;
    }
}

// Squared distance from the query to a child box of a fast node, in the units the planes are stored in, from the box's three plane words of the POSITIVE group
// (min | max << 16; a point has no direction): the three clamped differences and their squares in binary64. `ps` = P times the planes' power-of-two scale: exact.
// The caller multiplies by k = (1 / scale)^2 * (1 - 2^-48). Conservative for every finite P (DESIGN.md "Nearest-surface queries" has the argument): the planes were
// rounded OUTWARD, widening a binary16 is exact, each difference, square and sum is one rounding of relative size u = 2^-53 on non-negative terms -- so the computed
// sum is at most (1 + u)^5 times the exact squared distance to the box, nothing overflows (|ps| < 2^128, its square < 2^257) and nothing underflows (a difference of
// two such numbers is 0 or at least 2^-173) -- and a triangle's D2 is e = P - Q rounded, squared and summed, at least (1 - u)^5 times |P - Q|^2 with Q inside the box;
// (1 + u)^6 (1 - 32 u) < (1 - u)^5 leaves the margin. (1 - 2^-50 = 1 - 8 u would not: 1 - 2 u against 1 - 5 u.)
TD double nearest_box_bound ( uint32_t wx, uint32_t wy, uint32_t wz, D3 ps ) {
    const terra_half2 x = as_half2 ( wx ), y = as_half2 ( wy ), z = as_half2 ( wz );      // (min, max)
    const double dx = __builtin_fmax ( __builtin_fmax ( ( double ) x.x - ps.x, ps.x - ( double ) x.y ), 0.0 );
    const double dy = __builtin_fmax ( __builtin_fmax ( ( double ) y.x - ps.y, ps.y - ( double ) y.y ), 0.0 );
    const double dz = __builtin_fmax ( __builtin_fmax ( ( double ) z.x - ps.z, ps.z - ( double ) z.y ), 0.0 );
    return ( dx * dx + dy * dy ) + dz * dz;
}
// compare-exchange of two (bound, child word) pairs: afterwards a holds the smaller bound
TD void order_bound ( double& ka, uint32_t& ca, double& kb, uint32_t& cb ) {
    const bool swap = kb < ka;
    const double k0 = swap ? kb : ka, k1 = swap ? ka : kb; const uint32_t c0 = swap ? cb : ca, c1 = swap ? ca : cb;
    ka = k0; kb = k1; ca = c0; cb = c1;
}

template <int FAST>
__global__ __launch_bounds__ ( 256 ) void terra_nearest_kernel ( DevNearestParams p, const float4* queries, uint32_t n, float4* out, uint32_t* spill ) {
    extern __shared__ int words[];
    const uint32_t tid = threadIdx.x;
    const float4* tris = reinterpret_cast<const float4*> ( FAST ? p.scene.fast_tris : p.scene.tris );
    // (n <= 2^31 - 1 and the grid has at most 2^19 lanes: neither base + tid nor the stride's add leaves 32 bits)
    for ( uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u ) {          // (uniform in the block: the brute force's barriers are met by every lane)
        const uint32_t i = base + tid;
        const bool live = i < n;
        const float4 q = live ? queries[i] : make_float4 ( 0.f, 0.f, 0.f, -1.f );          // {position, max_distance}
        const D3 P = widen ( q );
        const double R = ( double ) q.w;
        // R NaN, +inf or >= FLT_MAX: no limit; R < 0, or a position that is not finite: nothing counts (r2 = -1: no D2 is <= it)
        const bool finite = __builtin_fabsf ( q.x ) <= FLT_MAX && __builtin_fabsf ( q.y ) <= FLT_MAX && __builtin_fabsf ( q.z ) <= FLT_MAX;
        const double r2 = ( !live || !finite || q.w < 0.f ) ? -1.0 : ( q.w < FLT_MAX ? R * R : __builtin_inf() );
        NearestBest best; best.d2 = __builtin_inf(); best.object = 0xffffffffu; best.triangle = 0xffffffffu; best.at = 0u;
        if ( FAST ) {
            if ( r2 >= 0.0 ) {
                const Tracer T = unstaged_tracer ( p.scene, words, p.stack_depth, 0, spill, p.spill_cap );
                const char* nodes = reinterpret_cast<const char*> ( p.scene.fast_nodes_h );
                const double inv = ( double ) p.scene.fast_inv_scale, scale = 1.0 / inv;          // powers of two: exact
                const D3 ps = dmul ( P, scale );
                const double k = ( inv * inv ) * ( 1.0 - 0x1p-48 );
                int* top = T.stack;
                uint32_t cur = 0u;                                                                // the root in hand, an empty stack
                for ( ;; ) {
                    if ( cur == DEV_CHILD_EMPTY ) { if ( top == T.stack ) break; cur = fast_pop ( T, top ); }
                    if ( ( int ) cur >= 0 ) {
                        const uint32_t off = cur << 7;
                        const uint4 gx = *reinterpret_cast<const uint4*> ( nodes + off ), gy = *reinterpret_cast<const uint4*> ( nodes + ( off + 32u ) ),
                                    gz = *reinterpret_cast<const uint4*> ( nodes + ( off + 64u ) ), ch = *reinterpret_cast<const uint4*> ( nodes + ( off + 96u ) );      // the positive groups {x0 x1 x2 x3} {y0 ..} {z0 ..} {children}
                        const double bound = best.d2 < r2 ? best.d2 : r2;
                        // an empty slot is an inverted box with FINITE planes: with no limit and no candidate yet the bound is +inf and the distance test would let
                        // it pass, so the child word decides. A child whose lower bound EQUALS the bound stays (the tie rule).
                        const double inf = __builtin_inf();
                        double k0 = nearest_box_bound ( gx.x, gy.x, gz.x, ps ) * k, k1 = nearest_box_bound ( gx.y, gy.y, gz.y, ps ) * k,
                               k2 = nearest_box_bound ( gx.z, gy.z, gz.z, ps ) * k, k3 = nearest_box_bound ( gx.w, gy.w, gz.w, ps ) * k;
                        uint32_t c0 = ch.x, c1 = ch.y, c2 = ch.z, c3 = ch.w;
                        if ( c0 == DEV_CHILD_EMPTY || k0 > bound ) { c0 = DEV_CHILD_EMPTY; k0 = inf; }
                        if ( c1 == DEV_CHILD_EMPTY || k1 > bound ) { c1 = DEV_CHILD_EMPTY; k1 = inf; }
                        if ( c2 == DEV_CHILD_EMPTY || k2 > bound ) { c2 = DEV_CHILD_EMPTY; k2 = inf; }
                        if ( c3 == DEV_CHILD_EMPTY || k3 > bound ) { c3 = DEV_CHILD_EMPTY; k3 = inf; }
                        // nearest first: a kept child's bound is finite (see nearest_box_bound: no overflow), so the culled ones, at +inf, sort last
                        order_bound ( k0, c0, k1, c1 ); order_bound ( k2, c2, k3, c3 ); order_bound ( k0, c0, k2, c2 ); order_bound ( k1, c1, k3, c3 ); order_bound ( k1, c1, k2, c2 );
                        if ( c3 != DEV_CHILD_EMPTY ) fast_push ( T, top, c3 );
                        if ( c2 != DEV_CHILD_EMPTY ) fast_push ( T, top, c2 );
                        if ( c1 != DEV_CHILD_EMPTY ) fast_push ( T, top, c1 );
                        cur = c0;
                    } else {
                        const uint32_t first = cur & 0x07ffffffu, count = ( ( cur >> 27 ) & 0xfu ) + 1u;
                        for ( uint32_t j = 0; j < count; ++j ) {
                            const uint32_t ti = first + j;
                            const float4 a = tris[3 * ( size_t ) ti], b = tris[3 * ( size_t ) ti + 1], c = tris[3 * ( size_t ) ti + 2];
                            D3 Q; uint32_t feature;
                            const double d2 = nearest_on_triangle ( widen ( a ), widen ( b ), widen ( c ), P, Q, feature );
                            nearest_take ( best, d2, r2, __float_as_uint ( a.w ), __float_as_uint ( b.w ), ti );
                        }
                        cur = DEV_CHILD_EMPTY;
                    }
                }
            }
        } else {
            float4* tile = reinterpret_cast<float4*> ( words );
            for ( uint32_t t0 = 0; t0 < p.scene.n_tris; t0 += TERRA_NEAREST_TILE ) {
                const uint32_t m = p.scene.n_tris - t0 < TERRA_NEAREST_TILE ? p.scene.n_tris - t0 : TERRA_NEAREST_TILE;
                __syncthreads();                                                                  // the tile before this one has been read by every lane
                if ( tid < m ) { const size_t s = 3 * ( size_t ) ( t0 + tid ); tile[3 * tid] = tris[s]; tile[3 * tid + 1] = tris[s + 1]; tile[3 * tid + 2] = tris[s + 2]; }
                __syncthreads();
                if ( r2 >= 0.0 ) for ( uint32_t j = 0; j < m; ++j ) {
                    const float4 a = tile[3 * j], b = tile[3 * j + 1], c = tile[3 * j + 2];
                    D3 Q; uint32_t feature;
                    const double d2 = nearest_on_triangle ( widen ( a ), widen ( b ), widen ( c ), P, Q, feature );
                    nearest_take ( best, d2, r2, __float_as_uint ( a.w ), __float_as_uint ( b.w ), t0 + j );
                }
            }
        }
        if ( !live ) continue;
        float4 h0 = make_float4 ( FLT_MAX, __uint_as_float ( 0xffffffffu ), __uint_as_float ( 0u ), __uint_as_float ( 0u ) ), h1 = make_float4 ( FLT_MAX, FLT_MAX, FLT_MAX, 0.f );
        if ( best.object != 0xffffffffu ) {
            // the record: the rule once more on the winner
            const float4 a = tris[3 * ( size_t ) best.at], b = tris[3 * ( size_t ) best.at + 1], c = tris[3 * ( size_t ) best.at + 2];
            const D3 A = widen ( a ), B = widen ( b ), C = widen ( c );
            D3 Q; uint32_t feature;
            const double d2 = nearest_on_triangle ( A, B, C, P, Q, feature );
            const D3 ab = dsub ( B, A ), ac = dsub ( C, A ), e = dsub ( P, Q );
            const D3 nrm = d3 ( ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x );
            const double s = ddot ( nrm, e );
            h0 = make_float4 ( ( float ) __builtin_sqrt ( d2 ), __uint_as_float ( best.object ), __uint_as_float ( best.triangle ), __uint_as_float ( feature ) );
            h1 = make_float4 ( ( float ) Q.x, ( float ) Q.y, ( float ) Q.z, s > 0.0 ? 1.f : s < 0.0 ? -1.f : 0.f );
        }
        out[2 * ( size_t ) i] = h0;
        out[2 * ( size_t ) i + 1] = h1;
    }
}

template <int FAST>
static hipError_t launch_nearest ( const DevNearestParams& p, const float4* queries, uint32_t n, float4* out, uint32_t* spill, uint32_t grid, size_t lds, hipStream_t stream ) {
    if ( lds > ( size_t ) 64 * 1024 ) {          // a stack padded by the test hook: opt in, as the ray query's launcher does
        const hipError_t e = hipFuncSetAttribute ( reinterpret_cast<const void*> ( terra_nearest_kernel<FAST> ), hipFuncAttributeMaxDynamicSharedMemorySize, ( int ) lds );
        if ( e != hipSuccess ) return e;
    }
    hipLaunchKernelGGL ( ( terra_nearest_kernel<FAST> ), dim3 ( grid ), dim3 ( 256 ), lds, stream, p, queries, n, out, spill );
    return hipGetLastError();
}

hipError_t terra_launch_nearest ( DevNearestParams p, const void* queries, size_t n, void* out, hipStream_t stream ) {
    if ( n == 0 ) return hipSuccess;
    if ( n > 0x7fffffffull ) return hipErrorInvalidValue;
    const uint64_t blocks = ( n + 255 ) / 256, cap = ( uint64_t ) terra_cu_count() * TERRA_NEAREST_MAX_BLOCKS_PER_CU;
    const uint32_t grid = ( uint32_t ) ( blocks < cap ? blocks : cap );
    // fast tree: the stack as the ray query has it -- the LDS column + HBM rest came with p (launch_plan.h terra_plan_fast_tree); brute force: one tile of triangles
    if ( p.fast && p.stack_depth < 1 ) p.stack_depth = 1;
    const size_t lds = p.fast ? ( size_t ) p.stack_depth * 1024 : ( size_t ) TERRA_NEAREST_TILE * 48;
    if ( lds > terra_lds_block_limit() ) return hipErrorInvalidValue;          // (terra_plan_fast_tree keeps at most TERRA_FAST_STACK_LDS entries in LDS; the pad hook may add to them)
    uint32_t* spill = nullptr;
    const size_t spill_bytes = p.fast ? terra_spill_bytes ( grid, p.spill_cap ) : 0;      // sized for the grid, not for n
    if ( spill_bytes ) { const hipError_t e = hipMallocAsync ( ( void** ) &spill, spill_bytes, stream ); if ( e != hipSuccess ) return e; }
    const float4* in = reinterpret_cast<const float4*> ( queries );
    const hipError_t e = p.fast ? launch_nearest<1> ( p, in, ( uint32_t ) n, reinterpret_cast<float4*> ( out ), spill, grid, lds, stream )
                                : launch_nearest<0> ( p, in, ( uint32_t ) n, reinterpret_cast<float4*> ( out ), spill, grid, lds, stream );
    if ( spill ) ( void ) hipFreeAsync ( spill, stream );          // stream-ordered: the kernel that uses it runs first
    return e;
}
