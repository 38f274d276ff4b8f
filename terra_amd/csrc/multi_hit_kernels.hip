// multi_hit_kernels.hip -- multi-hit ray queries on a committed scene (include/terra_amd.h "Multi-hit ray queries"; DESIGN.md "Multi-hit ray queries"): the first K
// triangles along each of a client's rays, or the number of triangles it crosses, read from and answered into HBM. A unit of its own: it takes no part in a render
// launch and shares no kernel with the ray queries or the nearest-surface queries.
//
// The launch shape is that of query_kernels.hip: one lane per ray, 256-lane blocks on a capped grid that strides over the rays, a ray read as two float4, a hit
// record written as two float4. A triangle COUNTS if the traversal's own watertight test (tri_perm / watertight_permuted: the same arithmetic, the same depth bits)
// accepts it at a depth <= the ray's limit L. terra_multi_hit_kernel<FAST, K>:
//   FAST = 1  a walk of the fast tree with the mechanics of traverse_fast_resume (traverse_fast.h: hand / held, the vote between node and triangle steps, the
//             nearest-first sort, fast_push / fast_pop on the LDS column + HBM spill, slab_half) -- MODE 2 and 3 scenes alike, with no reference_reaches replay: the
//             rule counts ANY triangle the test accepts, and the fast tree finds every one of them (DESIGN.md "Fast tree"). The cull is weaker than a closest-hit
//             walk's, so more entries are pushed; the stack bound does not depend on what is culled (at most three pushes per node step whatever the cut;
//             tree_build.cpp fastbvh::widen computes max_stack with every box entered), so terra_plan_fast_tree's plan holds unchanged.
//   FAST = 0  brute force, O(n * triangles): a block stages tiles of 256 soup triangles in LDS and every lane tests every triangle of the tile (all lanes read
//             the same LDS address: a broadcast). It serves the scenes without a fast tree; the soup's DevTri::pad is the rank in every scene (scene_host.cpp flatten).
//   K = 1, 2, 4, 8  the lane keeps a list of K (key, triangle) entries sorted by key = depth bits << 32 | rank: an accepted depth is >= 0 (watertight_permuted: the
//             numerator has the determinant's sign or is a zero; a NaN or an infinity fails depth <= L), and + 0.f turns -0 into +0, so the bits order like the
//             floats and ONE 64-bit compare per slot orders (depth, rank). Keys are distinct: ranks are a permutation and every triangle is in exactly one leaf.
//             A candidate enters if its key is below the last entry's (an empty slot is all ones, above every key) and sinks in by K compare-exchanges; the list
//             is indexed by unrolled constants only, so it lives in registers. The cut of the box test is the next float above min ( L, depth of the last entry ):
//             a box that starts at exactly the K-th depth is still entered, so a triangle that ties it in depth and beats it in rank still reaches the list. A
//             client's K is rounded up to the next instantiated length and only the first K records are written.
//   K = 0     counting: the cut stays at L and the lane counts. Every triangle is in exactly one leaf of the fast tree -- the host builder partitions the primitive
//             range at every split and a leaf is a run of that range (tree_build.cpp fastbvh::build), the device builder's leaves are runs of the sorted key
//             order (tree_build_device.hip), and widening only regroups child words --, so nothing is counted twice.
// The list holds keys, not depths: the records are made by testing the listed triangles once more, so `t` has the test's own bits (-0 included). No atomics: the
// same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "trace_device.h"
#include "kernels.h"
#include "launch_plan.h"

#define TERRA_MULTI_MAX_BLOCKS_PER_CU 8
#define TERRA_MULTI_TILE 256                  // triangles of a brute-force tile: one per lane of the block, 12 KB of LDS
#define TERRA_MULTI_NO_KEY 0xffffffffffffffffull
#define TERRA_MULTI_NO_TRI 0xffffffffu

template <int K> struct MultiHits { uint64_t key[K > 0 ? K : 1]; uint32_t tri[K > 0 ? K : 1]; uint32_t total; };
template <int K> TD MultiHits<K> multi_none() {
    MultiHits<K> h; h.total = 0u;
#pragma unroll
    for ( int j = 0; j < ( K > 0 ? K : 1 ); ++j ) { h.key[j] = TERRA_MULTI_NO_KEY; h.tri[j] = TERRA_MULTI_NO_TRI; }
    return h;
}
// a triangle the test accepted at `depth`: it counts if depth <= limit (false for a NaN); `at` = where its record is in the array the kernel reads
template <int K> TD void multi_take ( MultiHits<K>& h, float depth, float limit, uint32_t rank, uint32_t at ) {
    if ( ! ( depth <= limit ) ) return;
    if constexpr ( K == 0 ) ++h.total;
    else {
        uint64_t ck = ( ( uint64_t ) __float_as_uint ( depth + 0.f ) << 32 ) | rank; uint32_t ct = at;
        if ( ck < h.key[K - 1] ) {
#pragma unroll
            for ( int j = 0; j < K; ++j ) {          // the candidate sinks in; what falls off the end is dropped
                const bool lower = ck < h.key[j];
                const uint64_t k0 = lower ? ck : h.key[j], k1 = lower ? h.key[j] : ck; const uint32_t t0 = lower ? ct : h.tri[j], t1 = lower ? h.tri[j] : ct;
                h.key[j] = k0; h.tri[j] = t0; ck = k1; ct = t1;
            }
        }
    }
}
// the box test's cut: the next float above the depth nothing beyond which can count (limit is >= +0 and <= FLT_MAX: FLT_MAX -> inf)
template <int K> TD float multi_limit_up ( const MultiHits<K>& h, float limit ) {
    uint32_t cut = __float_as_uint ( limit );
    if constexpr ( K > 0 ) { const uint32_t last = ( uint32_t ) ( h.key[K - 1] >> 32 ); cut = last < cut ? last : cut; }      // (an empty slot: 0xffffffff)
    return __uint_as_float ( cut + 1u );
}

// The walk of the fast tree: traverse_fast_resume's loop (traverse_fast.h has the account of hand, held and the vote) run to the end of every lane's ray, with the
// list or the counter in place of the closest hit. A lane that is not active starts with nothing in hand and takes no step.
template <int K>
TD void multi_walk ( const Tracer& T, const Ray& ray, const RayState& st, V3 o_perm, float limit, bool active, MultiHits<K>& h ) {
    const FastRay f = fast_ray ( ray, T.sc.fast_inv_scale );
    const char* nodes = reinterpret_cast<const char*> ( T.sc.fast_nodes_h );
    const float4* tris = reinterpret_cast<const float4*> ( T.sc.fast_tris );
    int* top = T.stack;
    uint32_t hand = active ? TERRA_FAST_ROOT_IN_HAND : DEV_CHILD_EMPTY, held = 0u;
    for ( ;; ) {
        const uint64_t m_hold = __builtin_amdgcn_ballot_w64 ( held != 0u ), m_can = __builtin_amdgcn_ballot_w64 ( ( int ) hand >= 0 ) | ( __builtin_amdgcn_ballot_w64 ( hand == DEV_CHILD_EMPTY ) & __builtin_amdgcn_ballot_w64 ( top != T.stack ) );
        const int n_can = __popcll ( m_can ), n_hold = __popcll ( m_hold ), n_busy = __popcll ( m_can | m_hold );
        if ( n_busy == 0 ) break;
        if ( n_can != 0 && n_hold * 16 < n_busy * TERRA_FAST_LEAF_16THS ) {
            if ( ( ( int ) hand >= 0 ) | ( ( hand == DEV_CHILD_EMPTY ) & ( top != T.stack ) ) ) {
                uint32_t w = hand;
                if ( ( int ) w < 0 ) w = fast_pop ( T, top );
                uint32_t nw = w;                                     // (a leaf that waited on the stack stays in hand)
                if ( ( int ) w >= 0 ) {
                    const uint32_t off = w << 7;
                    const uint4 gx = *reinterpret_cast<const uint4*> ( nodes + ( off + f.px ) ), gy = *reinterpret_cast<const uint4*> ( nodes + ( off + f.py ) ),
                                gz = *reinterpret_cast<const uint4*> ( nodes + ( off + f.pz ) ), ch = *reinterpret_cast<const uint4*> ( nodes + ( off + 96u ) );
                    const float limit_up = multi_limit_up ( h, limit );
                    float te0, te1, te2, te3;
                    const bool hit0 = slab_half ( gx.x, gy.x, gz.x, f, limit_up, te0 );
                    const bool hit1 = slab_half ( gx.y, gy.y, gz.y, f, limit_up, te1 );
                    const bool hit2 = slab_half ( gx.z, gy.z, gz.z, f, limit_up, te2 );
                    const bool hit3 = slab_half ( gx.w, gy.w, gz.w, f, limit_up, te3 );
                    uint32_t k0 = hit0 ? __float_as_uint ( te0 ) : 0xffffffffu, k1 = hit1 ? __float_as_uint ( te1 ) : 0xffffffffu, k2 = hit2 ? __float_as_uint ( te2 ) : 0xffffffffu, k3 = hit3 ? __float_as_uint ( te3 ) : 0xffffffffu;
                    uint32_t c0 = ch.x, c1 = ch.y, c2 = ch.z, c3 = ch.w;
                    order_pair ( k0, c0, k1, c1 ); order_pair ( k2, c2, k3, c3 ); order_pair ( k0, c0, k2, c2 ); order_pair ( k1, c1, k3, c3 ); order_pair ( k1, c1, k2, c2 );
                    if ( k3 != 0xffffffffu ) fast_push ( T, top, c3 );          // at most three pushes per node step, whatever the cut let through
                    if ( k2 != 0xffffffffu ) fast_push ( T, top, c2 );
                    if ( k1 != 0xffffffffu ) fast_push ( T, top, c1 );
                    nw = k0 != 0xffffffffu ? c0 : DEV_CHILD_EMPTY;
                }
                { const bool take = ( ( int ) nw < -1 ) & ( held == 0u ); held = take ? nw : held; nw = take ? DEV_CHILD_EMPTY : nw; }
                hand = nw;
            }
        } else if ( held != 0u ) {
            const uint32_t ti = held & 0x07ffffffu;
            held = ( held & 0x78000000u ) ? held + 1u - 0x08000000u : 0u;
            if ( ( held == 0u ) & ( ( int ) hand < -1 ) ) { held = hand; hand = DEV_CHILD_EMPTY; }
            const float4 a = tris[3 * ti], b = tris[3 * ti + 1], cc = tris[3 * ti + 2];
            float depth;
            if ( watertight_permuted ( tri_perm ( a, b, cc, st ), o_perm, st, depth ) ) multi_take ( h, depth, limit, __float_as_uint ( cc.w ), ti );
        }
    }
}

// counts: K > 0: records written per ray (may be nullptr); K = 0: the crossing count per ray. kc = the client's K (<= K), the records of a ray side by side
template <int FAST, int K>
__global__ __launch_bounds__ ( 256 ) void terra_multi_hit_kernel ( DevMultiHitParams p, const float4* rays, uint32_t n, uint32_t kc, float4* out, uint32_t* counts, uint32_t* spill ) {
    extern __shared__ int words[];
    const uint32_t tid = threadIdx.x;
    const float4* tris = reinterpret_cast<const float4*> ( FAST ? p.scene.fast_tris : p.scene.tris );
    // (n <= 2^31 - 1 and the grid has at most 2^19 lanes: neither base + tid nor the stride's add leaves 32 bits)
    for ( uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u ) {          // (uniform in the block: the brute force's barriers are met by every lane)
        const uint32_t i = base + tid;
        const bool live = i < n;
        const float4 q0 = live ? rays[2 * ( size_t ) i] : make_float4 ( 0.f, 0.f, 0.f, -1.f ), q1 = live ? rays[2 * ( size_t ) i + 1] : make_float4 ( 0.f, 0.f, 1.f, 0.f );          // {origin, tmax} {direction, reserved}
        const Ray r = make_ray ( v3 ( q0.x, q0.y, q0.z ), v3 ( q1.x, q1.y, q1.z ) );
        const float limit = ( q0.w < FLT_MAX ? q0.w : FLT_MAX ) + 0.f;                                  // +inf, FLT_MAX and NaN: no limit; -0 is +0
        const float big = __builtin_fmaxf ( __builtin_fmaxf ( __builtin_fmaxf ( __builtin_fabsf ( q0.x ), __builtin_fabsf ( q0.y ) ), __builtin_fabsf ( q0.z ) ),
                                            __builtin_fmaxf ( __builtin_fmaxf ( __builtin_fabsf ( q1.x ), __builtin_fabsf ( q1.y ) ), __builtin_fabsf ( q1.z ) ) );
        const bool finite = q0.x == q0.x && q0.y == q0.y && q0.z == q0.z && q1.x == q1.x && q1.y == q1.y && q1.z == q1.z && big <= FLT_MAX;          // (fmax drops a NaN: asked for by itself)
        const bool zero = q1.x == 0.f && q1.y == 0.f && q1.z == 0.f;
        // inactive -- a zero direction, a component that is not finite --, a negative limit, a lane past the end: nothing counts, decided before any traversal
        const bool active = live && finite && !zero && limit >= 0.f;
        const RayState st = ray_state_init ( r );
        const V3 o_perm = permuted ( r.o, st );
        MultiHits<K> h = multi_none<K>();
        if ( FAST ) {
            const Tracer T = unstaged_tracer ( p.scene, words, p.stack_depth, 0, spill, p.spill_cap );
            multi_walk<K> ( T, r, st, o_perm, limit, active, h );
        } else {
            float4* tile = reinterpret_cast<float4*> ( words );
            for ( uint32_t t0 = 0; t0 < p.scene.n_tris; t0 += TERRA_MULTI_TILE ) {
                const uint32_t m = p.scene.n_tris - t0 < TERRA_MULTI_TILE ? p.scene.n_tris - t0 : TERRA_MULTI_TILE;
                __syncthreads();                                                                  // the tile before this one has been read by every lane
                if ( tid < m ) { const size_t s = 3 * ( size_t ) ( t0 + tid ); tile[3 * tid] = tris[s]; tile[3 * tid + 1] = tris[s + 1]; tile[3 * tid + 2] = tris[s + 2]; }
                __syncthreads();
                if ( active ) for ( uint32_t j = 0; j < m; ++j ) {
                    const float4 a = tile[3 * j], b = tile[3 * j + 1], cc = tile[3 * j + 2];
                    float depth;
                    if ( watertight_permuted ( tri_perm ( a, b, cc, st ), o_perm, st, depth ) ) multi_take ( h, depth, limit, __float_as_uint ( cc.w ), t0 + j );
                }
            }
        }
        if ( !live ) continue;
        if constexpr ( K == 0 ) counts[i] = h.total;
        else {
            float4* rec = out + 2 * ( ( size_t ) i * kc );
            uint32_t written = 0u;
#pragma unroll
            for ( int j = 0; j < K; ++j ) {
                if ( ( uint32_t ) j >= kc ) break;
                float4 h0 = make_float4 ( FLT_MAX, __uint_as_float ( 0xffffffffu ), __uint_as_float ( 0u ), 0.f ), h1 = make_float4 ( FLT_MAX, FLT_MAX, FLT_MAX, 0.f );
                if ( h.tri[j] != TERRA_MULTI_NO_TRI ) {
                    // the record: the test once more on the listed triangle (it accepted it before: the same operands, the same bits)
                    const size_t s = 3 * ( size_t ) h.tri[j];
                    const float4 a = tris[s], b = tris[s + 1], cc = tris[s + 2];
                    float depth = 0.f;
                    ( void ) watertight_permuted ( tri_perm ( a, b, cc, st ), o_perm, st, depth );
                    const V3 pt = r.o + r.d * depth;
                    h0 = make_float4 ( depth, a.w, b.w, 0.f );
                    h1 = make_float4 ( pt.x, pt.y, pt.z, 0.f );
                    ++written;
                }
                rec[2 * j] = h0; rec[2 * j + 1] = h1;
            }
            if ( counts ) counts[i] = written;
        }
    }
}

template <int FAST, int K>
static hipError_t launch_multi_hit ( const DevMultiHitParams& p, const float4* rays, uint32_t n, uint32_t kc, float4* out, uint32_t* counts, uint32_t* spill, uint32_t grid, size_t lds, hipStream_t stream ) {
    if ( lds > ( size_t ) 64 * 1024 ) {          // a stack padded by the test hook: opt in, as the ray query's launcher does
        const hipError_t e = hipFuncSetAttribute ( reinterpret_cast<const void*> ( terra_multi_hit_kernel<FAST, K> ), hipFuncAttributeMaxDynamicSharedMemorySize, ( int ) lds );
        if ( e != hipSuccess ) return e;
    }
    hipLaunchKernelGGL ( ( terra_multi_hit_kernel<FAST, K> ), dim3 ( grid ), dim3 ( 256 ), lds, stream, p, rays, n, kc, out, counts, spill );
    return hipGetLastError();
}
template <int FAST>
static hipError_t launch_multi_hit_k ( const DevMultiHitParams& p, const float4* rays, uint32_t n, uint32_t kc, float4* out, uint32_t* counts, uint32_t* spill, uint32_t grid, size_t lds, hipStream_t stream ) {
    // the client's K rounded up to the next list length there is a kernel for
    if ( kc == 0 ) return launch_multi_hit<FAST, 0> ( p, rays, n, kc, out, counts, spill, grid, lds, stream );
    if ( kc == 1 ) return launch_multi_hit<FAST, 1> ( p, rays, n, kc, out, counts, spill, grid, lds, stream );
    if ( kc == 2 ) return launch_multi_hit<FAST, 2> ( p, rays, n, kc, out, counts, spill, grid, lds, stream );
    if ( kc <= 4 ) return launch_multi_hit<FAST, 4> ( p, rays, n, kc, out, counts, spill, grid, lds, stream );
    return launch_multi_hit<FAST, 8> ( p, rays, n, kc, out, counts, spill, grid, lds, stream );
}

hipError_t terra_launch_multi_hit ( DevMultiHitParams p, const void* rays, size_t n, uint32_t k, void* hits, void* counts, hipStream_t stream ) {
    if ( n == 0 ) return hipSuccess;
    if ( n > 0x7fffffffull || k > 8u || ( k == 0 ? !counts : !hits ) ) return hipErrorInvalidValue;
    const uint64_t blocks = ( n + 255 ) / 256, cap = ( uint64_t ) terra_cu_count() * TERRA_MULTI_MAX_BLOCKS_PER_CU;
    const uint32_t grid = ( uint32_t ) ( blocks < cap ? blocks : cap );
    // fast tree: the stack as the ray query has it -- the LDS column + HBM rest came with p (launch_plan.h terra_plan_fast_tree; the weaker cut pushes more entries
    // than a closest-hit walk does, but the tree's fast_max_stack is the bound with EVERY box entered, so the plan covers it); brute force: one tile of triangles
    if ( p.fast && p.stack_depth < 1 ) p.stack_depth = 1;
    const size_t lds = p.fast ? ( size_t ) p.stack_depth * 1024 : ( size_t ) TERRA_MULTI_TILE * 48;
    if ( lds > terra_lds_block_limit() ) return hipErrorInvalidValue;
    uint32_t* spill = nullptr;
    const size_t spill_bytes = p.fast ? terra_spill_bytes ( grid, p.spill_cap ) : 0;      // sized for the grid, not for n
    if ( spill_bytes ) { const hipError_t e = hipMallocAsync ( ( void** ) &spill, spill_bytes, stream ); if ( e != hipSuccess ) return e; }
    const float4* in = reinterpret_cast<const float4*> ( rays );
    const hipError_t e = p.fast ? launch_multi_hit_k<1> ( p, in, ( uint32_t ) n, k, reinterpret_cast<float4*> ( hits ), reinterpret_cast<uint32_t*> ( counts ), spill, grid, lds, stream )
                                : launch_multi_hit_k<0> ( p, in, ( uint32_t ) n, k, reinterpret_cast<float4*> ( hits ), reinterpret_cast<uint32_t*> ( counts ), spill, grid, lds, stream );
    if ( spill ) ( void ) hipFreeAsync ( spill, stream );          // stream-ordered: the kernel that uses it runs first
    return e;
}
