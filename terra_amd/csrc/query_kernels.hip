// query_kernels.hip -- batched ray queries on a committed scene (include/terra_amd.h "Ray queries"; DESIGN.md "Ray queries"): closest hit and occlusion
// of a client's own rays, read from and answered into HBM.
//
// One lane per ray, 256-lane blocks on a capped grid that strides over the rays: consecutive lanes take consecutive rays, a lane reads its 32-byte ray as two
// float4 and writes its 32-byte hit as two float4 (closest hit) or one dword (occlusion), so every access of a wave is one contiguous run. The traversal is the
// one a render call of the scene takes (terra_launch_aov makes the same choice): the fast tree (MODE 2, or 3 with the reachability replay) or the reference tree
// read from global memory (MODE 0), with the leaf-box cull where the commit proved it. The ray is traced as given -- no origin offset: this is terra_bvh_traverse,
// not terra_scene_raycast -- and a triangle counts if the watertight test accepts it and its depth is <= the ray's limit L:
//   fast tree       the closest hit starts at (depth L, rank 0xffffffff), so every box beyond L is culled from the root on and "closer, or as close with a smaller
//                   rank" accepts a depth of exactly L (traverse_fast_resume: `best` is in / out);
//   reference tree  its traversal never culls against a hit, and keeps the first of equal depths by a strict "<": the closest hit starts at the next float above L.
// ANYHIT: the first triangle that counts ends the lane's traversal (traverse_fast_resume `anyhit`, leaf_step<.., ANYHIT>); in reachability mode only one the
// reference traversal reaches does (`checked`). A lane that is done idles until its wave's rays are done. No atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include "trace_device.h"
#include "kernels.h"
#include "launch_plan.h"

#define TERRA_QUERY_MAX_BLOCKS_PER_CU 8

template <int MODE, bool ANYHIT>
__global__ __launch_bounds__ ( 256 ) void terra_query_kernel ( DevQueryParams p, const float4* rays, uint32_t n, void* out, uint32_t* spill ) {
    extern __shared__ int words[];
    const uint32_t tid = threadIdx.x;
    Tracer T = unstaged_tracer ( p.scene, words, p.stack_depth, p.leaf_cap, spill, p.spill_cap );
    // (n <= 2^31 - 1 and the grid has at most 2^19 lanes: neither base + tid nor the stride's add leaves 32 bits)
    for ( uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u ) {
        const uint32_t i = base + tid;
        if ( i >= n ) continue;
        const float4 q0 = rays[2 * ( size_t ) i], q1 = rays[2 * ( size_t ) i + 1];          // {origin, tmax} {direction, reserved}
        const Ray r = make_ray ( v3 ( q0.x, q0.y, q0.z ), v3 ( q1.x, q1.y, q1.z ) );
        const float limit = q0.w < FLT_MAX ? q0.w : FLT_MAX;                                  // +inf, FLT_MAX and NaN: no limit
        float depth = FLT_MAX; uint32_t object = 0xffffffffu, triangle = 0u;
        if ( limit >= 0.f ) {                                                                  // (a negative limit: nothing counts)
            const RayState st = ray_state_init ( r );
            const V3 o_perm = permuted ( r.o, st );
            Counters c = counters_zero();
            if ( MODE == 0 ) {
                // the leaf-box cull holds for origins inside the range the commit verified (the render call asks the same of its camera): decided ray by ray
                T.cull = p.leaf_cull != 0 && fabsf ( r.o.x ) <= p.origin_limit && fabsf ( r.o.y ) <= p.origin_limit && fabsf ( r.o.z ) <= p.origin_limit;
                Closest best; best.tri = 0xffffffffu;
                best.depth = limit < FLT_MAX ? __uint_as_float ( __float_as_uint ( limit + 0.f ) + 1u ) : FLT_MAX;      // + 0.f: a limit of -0 is +0
                // (the slab variant is chosen per wave, as bvh_traverse chooses it)
                if ( __all ( ray_is_regular ( r ) ) ) traverse_loops<0, 0, true, false, ANYHIT> ( T, r, st, o_perm, best, c );
                else traverse_loops<0, 0, false, false, ANYHIT> ( T, r, st, o_perm, best, c );
                if ( best.tri != 0xffffffffu ) { depth = best.depth; object = p.scene.tris[best.tri].object; triangle = p.scene.tris[best.tri].tri_in_object; }
            } else {
                ClosestRanked best;
                // MODE 3, closest hit: the closest of ALL triangles that count is the answer if the reference reaches it; only if not is the ray traced again with
                // every candidate checked (bvh_traverse_fast). Occlusion checks every candidate in its one pass: an unchecked one must not end the search.
                for ( int pass = 0; pass < 2; ++pass ) {
                    best.depth = limit; best.rank = 0xffffffffu; best.tri = 0xffffffffu;
                    int* top = T.stack;
                    uint32_t hand = TERRA_FAST_ROOT_IN_HAND, held = 0u;
                    const bool checked = MODE == 3 && ( ANYHIT || pass == 1 );
                    traverse_fast_resume<0> ( T, r, st, o_perm, best, top, hand, held, 0, c, checked, ANYHIT );
                    if ( MODE != 3 || checked || best.tri == 0xffffffffu || reference_reaches ( T, best.tri, r ) ) break;
                }
                if ( best.tri != 0xffffffffu ) { depth = best.depth; object = p.scene.fast_tris[best.tri].object; triangle = p.scene.fast_tris[best.tri].tri_in_object; }
            }
        }
        const bool hit = object != 0xffffffffu;
        if ( ANYHIT ) reinterpret_cast<uint32_t*> ( out )[i] = hit ? 1u : 0u;
        else {
            const V3 pt = hit ? r.o + r.d * depth : v3 ( FLT_MAX, FLT_MAX, FLT_MAX );
            float4* h = reinterpret_cast<float4*> ( out ) + 2 * ( size_t ) i;
            h[0] = make_float4 ( depth, __uint_as_float ( object ), __uint_as_float ( triangle ), 0.f );
            h[1] = make_float4 ( pt.x, pt.y, pt.z, 0.f );
        }
    }
}

template <int MODE, bool ANYHIT>
static hipError_t launch_query ( const DevQueryParams& p, const float4* rays, uint32_t n, void* out, uint32_t* spill, uint32_t grid, size_t lds, hipStream_t stream ) {
    if ( lds > ( size_t ) 64 * 1024 ) {
        const hipError_t e = hipFuncSetAttribute ( reinterpret_cast<const void*> ( terra_query_kernel<MODE, ANYHIT> ), hipFuncAttributeMaxDynamicSharedMemorySize, ( int ) lds );
        if ( e != hipSuccess ) return e;
    }
    hipLaunchKernelGGL ( ( terra_query_kernel<MODE, ANYHIT> ), dim3 ( grid ), dim3 ( 256 ), lds, stream, p, rays, n, out, spill );
    return hipGetLastError();
}

hipError_t terra_launch_query ( DevQueryParams p, const void* rays, size_t n, void* out, bool anyhit, hipStream_t stream ) {
    if ( n == 0 ) return hipSuccess;
    if ( n > 0x7fffffffull ) return hipErrorInvalidValue;
    const uint64_t blocks = ( n + 255 ) / 256, cap = ( uint64_t ) terra_cu_count() * TERRA_QUERY_MAX_BLOCKS_PER_CU;
    const uint32_t grid = ( uint32_t ) ( blocks < cap ? blocks : cap );
    // the stack as terra_launch_aov plans it: the fast tree's LDS column + HBM rest came with p (launch_plan.h terra_plan_fast_tree); the reference tree's whole
    // stack and a leaf list of what 64 KB leave (at least 4 entries) live in LDS (terra_unstaged_leaf_cap)
    int mode = 0;
    if ( p.fast ) mode = p.scene.reach ? 3 : 2;
    else { if ( p.stack_depth < 1 ) p.stack_depth = 1; p.leaf_cap = terra_unstaged_leaf_cap ( p.stack_depth, 0 ); p.spill_cap = 0; }
    const size_t lds = ( size_t ) ( p.stack_depth + ( mode == 0 ? p.leaf_cap : 0u ) ) * 1024;
    if ( lds > terra_lds_block_limit() ) return hipErrorInvalidValue;
    uint32_t* spill = nullptr;
    const size_t spill_bytes = mode != 0 ? terra_spill_bytes ( grid, p.spill_cap ) : 0;      // sized for the grid, not for n
    if ( spill_bytes ) { const hipError_t e = hipMallocAsync ( ( void** ) &spill, spill_bytes, stream ); if ( e != hipSuccess ) return e; }
    const float4* in = reinterpret_cast<const float4*> ( rays );
    const uint32_t n32 = ( uint32_t ) n;
    hipError_t e;
    if ( anyhit ) e = mode == 0 ? launch_query<0, true> ( p, in, n32, out, spill, grid, lds, stream ) : mode == 2 ? launch_query<2, true> ( p, in, n32, out, spill, grid, lds, stream ) : launch_query<3, true> ( p, in, n32, out, spill, grid, lds, stream );
    else          e = mode == 0 ? launch_query<0, false> ( p, in, n32, out, spill, grid, lds, stream ) : mode == 2 ? launch_query<2, false> ( p, in, n32, out, spill, grid, lds, stream ) : launch_query<3, false> ( p, in, n32, out, spill, grid, lds, stream );
    if ( spill ) ( void ) hipFreeAsync ( spill, stream );          // stream-ordered: the kernel that uses it runs first
    return e;
}
