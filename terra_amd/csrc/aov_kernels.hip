// aov_kernels.hip -- first-hit AOV buffers (include/terra_amd.h "AOV buffers"; DESIGN.md "AOV buffers and the denoiser"). The denoiser that reads them is
// denoise_kernels.hip.
//
// One camera ray per sample, nothing shaded. Sample n of a pixel traces exactly the camera ray sample n of the same pixel traces in the render:
// the same stream keys (pixel, samples already in the AOV pixel + chunk * chunk_spp), the same draws (r1, r2 from stream A, then the sampler integration's
// pair), the same sample split (scene_host.cpp launch_split) and the traversal the render call would take (fill_params). A 256-thread block holds 256 / split
// pixels x split chunks; the chunk sums meet in LDS and the chunk-0 lane of each pixel adds them to the buffer in chunk order -- what terra_resolve_kernel does.
// The grid is capped and strides over the blocks (the fast tree's stack spill is sized for the grid, not the frame).
//
// Compiled twice (terra_amd/build.py): as it stands, and with TERRA_TU=4 as the RAY-SOURCED unit (TERRA_RAY_SOURCE, dev_types.h; include/terra_amd.h "Ray-sourced
// rendering"), whose kernel terra_aov_rays_kernel and launcher terra_launch_aov_rays take a ray buffer -- one TerraAmdRay per pixel, addressed like the AOV buffer -- and trace the pixel's
// ray for every sample: depth sums |hit point - ray origin|, an inactive ray adds its samples and nothing else. The camera unit's code is the same with and without it.
// With TERRA_TU=8 it is the LENS unit (TERRA_RAY_SOURCE 2; include/terra_amd.h "Lens rendering"): terra_aov_lens_kernel and terra_launch_aov_lens trace, per sample, the
// ray lens_sample (trace_geometry.h) makes from the camera model, drawing stream A as the lens render kernels do; the unit also holds the generator's unit entry
// (terra_unit_lens_rays), so that no other unit's code changes.
// With TERRA_TU=12 it is the POINT unit (TERRA_RAY_SOURCE 3; include/terra_amd.h "Point rendering"): terra_aov_points_kernel and terra_launch_aov_points trace, per
// sample, the ray point_sample (trace_geometry.h) draws about the pixel's point, drawing stream A as the point render kernels do; the unit also holds the generator's
// unit entry (terra_unit_point_rays).
#include <hip/hip_runtime.h>
#include "trace_device.h"
#include "kernels.h"
#include "launch_plan.h"

struct DevAov { float albedo[3]; float coverage; float normal[3]; float depth; int samples; int reserved[3]; };      // TerraAmdAovResult
static_assert ( sizeof ( DevAov ) == 48, "DevAov must be 48 bytes" );

// ---- AOV pass ----------------------------------------------------------------------------------------------------------
#define TERRA_AOV_FOLD_BYTES ( 2 * 256 * 16 )       // the block's chunk sums: two float4 per lane
#define TERRA_AOV_MAX_BLOCKS_PER_CU 8

#if TERRA_RAY_SOURCE == 3
#define TERRA_AOV_KERNEL terra_aov_points_kernel
#define TERRA_AOV_RAYS_PARAM , const float4* points, const DevPointSampling sampling
#elif TERRA_RAY_SOURCE == 2
#define TERRA_AOV_KERNEL terra_aov_lens_kernel
#define TERRA_AOV_RAYS_PARAM , const DevLens lens
#elif TERRA_RAY_SOURCE == 1
#define TERRA_AOV_KERNEL terra_aov_rays_kernel
#define TERRA_AOV_RAYS_PARAM , const float4* rays
#else
#define TERRA_AOV_KERNEL terra_aov_kernel
#define TERRA_AOV_RAYS_PARAM , const uint32_t* mask      // masked launches (include/terra_amd.h "Masked rendering"): one word per 16x16 block of the rectangle, row-major as the blocks here are; nullptr: none
#endif
template <int MODE>
__global__ __launch_bounds__ ( 256 ) void TERRA_AOV_KERNEL ( DevRenderParams p, float4* aov, uint32_t* spill, uint32_t vblocks, uint32_t blocks_x TERRA_AOV_RAYS_PARAM ) {
    extern __shared__ float4 lds_f4[];
    const uint32_t tid = threadIdx.x;
    float4* fold = lds_f4;
    int* words = reinterpret_cast<int*> ( lds_f4 + 512 );
    Tracer T = unstaged_tracer ( p.scene, words, p.stack_depth, p.leaf_cap, spill, p.spill_cap );
    T.cull = p.leaf_cull != 0;
    const V3 cam_pos = v3 ( p.cam_pos[0], p.cam_pos[1], p.cam_pos[2] );
    const uint32_t ppb_log2 = 8u - p.split_log2, ppb = 1u << ppb_log2;          // pixels per block
    const uint32_t chunk = tid >> ppb_log2, k = tid & ( ppb - 1u );
    for ( uint32_t vb = blockIdx.x; vb < vblocks; vb += gridDim.x ) {
        // virtual block vb = part (vb mod split) of 16x16 pixel block vb / split of the rectangle; a wave covers an 8x8 packet as in the render (block_pixel)
        const uint32_t blk = vb >> p.split_log2, r = ( ( vb & ( p.split - 1u ) ) << ppb_log2 ) + k;
#if TERRA_RAY_SOURCE == 0
        if ( mask && mask[blk] == 0u ) continue;          // an inactive block is left alone (uniform over the thread block: nobody waits at the barriers below)
#endif
        const uint32_t by = blk / blocks_x, bx = blk - by * blocks_x;
        const uint32_t wave = r >> 6, lane = r & 63u;
        const uint32_t lx = bx * 16u + ( wave & 1u ) * 8u + ( lane & 7u ), ly = by * 16u + ( wave >> 1 ) * 8u + ( lane >> 3 );
        const bool inside = lx < p.w && ly < p.h;
        const uint32_t px = p.x + lx, py = p.y + ly;
        const size_t pix = inside ? ( size_t ) ( py - p.st_y ) * p.st_pitch + ( px - p.st_x ) : 0;
        float4 s0 = make_float4 ( 0.f, 0.f, 0.f, 0.f ), s1 = make_float4 ( 0.f, 0.f, 0.f, 0.f );
#if TERRA_RAY_SOURCE == 3
        if ( inside ) {
            // the camera form below with the point launch's ray: r1, r2 (unused), the sampler integration's pair, then g1, g2; an inactive point adds its samples and nothing else
            const float4* rec = points + 2 * pix;
            const float4 q0 = rec[0], q1 = rec[1];          // {position, reserved} {normal, reserved2}
            const V3 pos = v3 ( q0.x, q0.y, q0.z ), nrm = v3 ( q1.x, q1.y, q1.z );
            if ( !point_inactive ( pos, nrm ) ) {
                const int prior = __float_as_int ( aov[3 * pix + 2].x );
                const uint32_t base = ( uint32_t ) prior + chunk * p.chunk_spp;
                PixelStreams rs = trng_pixel_streams ( p.frame_seed, ( uint64_t ) py * p.fb_w + px, ( uint64_t ) ( uint32_t ) prior + ( uint64_t ) chunk * p.chunk_spp );
                for ( uint32_t s = 0; s < p.chunk_spp; ++s ) {
                    ( void ) trng_a_float ( rs.a ); ( void ) trng_a_float ( rs.a );
                    if ( p.sampler_mode ) ( void ) sampler_pair_draw ( p.sampler_mode, p.sampler_strata, ( uint64_t ) base + s, rs.a );
                    const float g1 = trng_a_float ( rs.a ), g2 = trng_a_float ( rs.a );
                    V3 ro, rd;
                    point_sample ( sampling, pos, nrm, g1, g2, ro, rd );
                    Surface sf;
                    Counters c = counters_zero();
                    const RaycastResult h = scene_raycast<0, MODE, TERRA_KINDS_ALL> ( T, make_ray ( ro, rd ), sf, c );
                    if ( h.hit ) {
                        const V3 a = sf.bsdf == kDevBsdfPhong ? sf.attr[1] : sf.attr[0];
                        s0.x = s0.x + a.x; s0.y = s0.y + a.y; s0.z = s0.z + a.z; s0.w = s0.w + 1.f;
                        s1.x = s1.x + sf.normal.x; s1.y = s1.y + sf.normal.y; s1.z = s1.z + sf.normal.z;
                        s1.w = s1.w + length ( ro - h.point );
                    }
                }
            }
        }
#elif TERRA_RAY_SOURCE == 2
        if ( inside ) {
            // the camera form below with the lens launch's ray: r1, r2, the sampler integration's pair, then the lens pair where the launch draws one
            const int prior = __float_as_int ( aov[3 * pix + 2].x );
            const uint32_t base = ( uint32_t ) prior + chunk * p.chunk_spp;
            PixelStreams rs = trng_pixel_streams ( p.frame_seed, ( uint64_t ) py * p.fb_w + px, ( uint64_t ) ( uint32_t ) prior + ( uint64_t ) chunk * p.chunk_spp );
            for ( uint32_t s = 0; s < p.chunk_spp; ++s ) {
                const float r1 = trng_a_float ( rs.a ), r2 = trng_a_float ( rs.a );
                if ( p.sampler_mode ) ( void ) sampler_pair_draw ( p.sampler_mode, p.sampler_strata, ( uint64_t ) base + s, rs.a );
                float l1 = 0.f, l2 = 0.f;
                if ( lens_draws ( lens ) ) { l1 = trng_a_float ( rs.a ); l2 = trng_a_float ( rs.a ); }
                V3 ro, rd;
                lens_sample ( p, lens, px, py, r1, r2, l1, l2, ro, rd );
                Surface sf;
                Counters c = counters_zero();
                const RaycastResult h = scene_raycast<0, MODE, TERRA_KINDS_ALL> ( T, make_ray ( ro, rd ), sf, c );
                if ( h.hit ) {
                    const V3 a = sf.bsdf == kDevBsdfPhong ? sf.attr[1] : sf.attr[0];
                    s0.x = s0.x + a.x; s0.y = s0.y + a.y; s0.z = s0.z + a.z; s0.w = s0.w + 1.f;
                    s1.x = s1.x + sf.normal.x; s1.y = s1.y + sf.normal.y; s1.z = s1.z + sf.normal.z;
                    s1.w = s1.w + length ( ro - h.point );
                }
            }
        }
#elif TERRA_RAY_SOURCE == 1
        if ( inside ) {
            // every sample of the pixel traces the pixel's ray (no draw decides anything here): one traversal, its hit added once per sample, in sample order
            const float4* rec = rays + 2 * pix;
            const float4 q0 = rec[0], q1 = rec[1];          // {origin, tmax} {direction, reserved}
            const V3 ro = v3 ( q0.x, q0.y, q0.z ), rd = v3 ( q1.x, q1.y, q1.z );
            const bool finite = fabsf ( ro.x ) < INFINITY && fabsf ( ro.y ) < INFINITY && fabsf ( ro.z ) < INFINITY && fabsf ( rd.x ) < INFINITY && fabsf ( rd.y ) < INFINITY && fabsf ( rd.z ) < INFINITY;
            if ( finite && ! ( rd.x == 0.f && rd.y == 0.f && rd.z == 0.f ) ) {          // (else: an inactive ray)
                Surface sf;
                Counters c = counters_zero();
                const RaycastResult h = scene_raycast<0, MODE, TERRA_KINDS_ALL> ( T, make_ray ( ro, rd ), sf, c );
                if ( h.hit ) {
                    const V3 a = sf.bsdf == kDevBsdfPhong ? sf.attr[1] : sf.attr[0];
                    const float dist = length ( ro - h.point );
                    for ( uint32_t s = 0; s < p.chunk_spp; ++s ) {
                        s0.x = s0.x + a.x; s0.y = s0.y + a.y; s0.z = s0.z + a.z; s0.w = s0.w + 1.f;
                        s1.x = s1.x + sf.normal.x; s1.y = s1.y + sf.normal.y; s1.z = s1.z + sf.normal.z;
                        s1.w = s1.w + dist;
                    }
                }
            }
        }
#else
        if ( inside ) {
            const int prior = __float_as_int ( aov[3 * pix + 2].x );
            const uint32_t base = ( uint32_t ) prior + chunk * p.chunk_spp;     // (job_next: j.base)
            PixelStreams rs = trng_pixel_streams ( p.frame_seed, ( uint64_t ) py * p.fb_w + px, ( uint64_t ) ( uint32_t ) prior + ( uint64_t ) chunk * p.chunk_spp );
            for ( uint32_t s = 0; s < p.chunk_spp; ++s ) {
                const float r1 = trng_a_float ( rs.a ), r2 = trng_a_float ( rs.a );
                const V3 rd = camera_sample ( p, px, py, r1, r2 );
                if ( p.sampler_mode ) ( void ) sampler_pair_draw ( p.sampler_mode, p.sampler_strata, ( uint64_t ) base + s, rs.a );      // (its stratified offsets are stream-A draws)
                Surface sf;
                Counters c = counters_zero();
                const RaycastResult h = scene_raycast<0, MODE, TERRA_KINDS_ALL> ( T, make_ray ( cam_pos, rd ), sf, c );
                if ( h.hit ) {
                    const V3 a = sf.bsdf == kDevBsdfPhong ? sf.attr[1] : sf.attr[0];     // TERRA_PHONG_ALBEDO; TERRA_DIFFUSE_ALBEDO, TERRA_GGX_F0, TERRA_GLASS_TINT are slot 0
                    s0.x = s0.x + a.x; s0.y = s0.y + a.y; s0.z = s0.z + a.z; s0.w = s0.w + 1.f;
                    s1.x = s1.x + sf.normal.x; s1.y = s1.y + sf.normal.y; s1.z = s1.z + sf.normal.z;
                    s1.w = s1.w + length ( cam_pos - h.point );                                 // (the DebugDepth integrator's distance, before its / 500)
                }
            }
        }
#endif
        fold[tid] = s0; fold[256 + tid] = s1;
        __syncthreads();
        if ( chunk == 0 && inside ) {
            float4 o0 = aov[3 * pix], o1 = aov[3 * pix + 1], o2 = aov[3 * pix + 2];
            for ( uint32_t j = 0; j < p.split; ++j ) {
                const float4 q0 = fold[j * ppb + k], q1 = fold[256 + j * ppb + k];
                o0.x = o0.x + q0.x; o0.y = o0.y + q0.y; o0.z = o0.z + q0.z; o0.w = o0.w + q0.w;
                o1.x = o1.x + q1.x; o1.y = o1.y + q1.y; o1.z = o1.z + q1.z; o1.w = o1.w + q1.w;
            }
            o2.x = __int_as_float ( __float_as_int ( o2.x ) + ( int ) p.spp );
            aov[3 * pix] = o0; aov[3 * pix + 1] = o1; aov[3 * pix + 2] = o2;
        }
        __syncthreads();
    }
}

#if TERRA_RAY_SOURCE == 3
// the generator on arrays (terra_amd_unit_point_rays): one thread per input; an inactive point gives the all-zero origin and direction
__global__ void k_point_rays ( DevPointSampling sampling, int n, const float4* points, const float* g2, float* rays8 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    const float4 q0 = points[2 * ( size_t ) i], q1 = points[2 * ( size_t ) i + 1];
    const V3 pos = v3 ( q0.x, q0.y, q0.z ), nrm = v3 ( q1.x, q1.y, q1.z );
    V3 ro = v3 ( 0.f, 0.f, 0.f ), rd = v3 ( 0.f, 0.f, 0.f );
    if ( !point_inactive ( pos, nrm ) ) point_sample ( sampling, pos, nrm, g2[2 * ( size_t ) i], g2[2 * ( size_t ) i + 1], ro, rd );
    float* q = rays8 + 8 * ( size_t ) i;
    q[0] = ro.x; q[1] = ro.y; q[2] = ro.z; q[3] = FLT_MAX;
    q[4] = rd.x; q[5] = rd.y; q[6] = rd.z; q[7] = 0.f;          // (reserved: the all-zero word)
}
hipError_t terra_unit_point_rays ( const DevPointSampling& sampling, int n, const float* points8, const float* g2, float* rays8 ) {
    if ( n <= 0 ) return hipSuccess;
    hipLaunchKernelGGL ( k_point_rays, dim3 ( ( n + 255 ) / 256 ), dim3 ( 256 ), 0, 0, sampling, n, reinterpret_cast<const float4*> ( points8 ), g2, rays8 );
    return hipGetLastError();
}
#define TERRA_AOV_RAYS_ARG , reinterpret_cast<const float4*> ( points ), sampling
hipError_t terra_launch_aov_points ( DevRenderParams p, const void* points, const DevPointSampling& sampling, void* aov, hipStream_t stream ) {
    if ( !points || sampling.distribution < 0 || sampling.distribution > 1 ) return hipErrorInvalidValue;
#elif TERRA_RAY_SOURCE == 2
// the generator on arrays (terra_amd_unit_lens_rays): one thread per input
__global__ void k_lens_rays ( DevRenderParams p, DevLens lens, int n, const uint32_t* xy2, const float* r4, float* rays8 ) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    V3 ro, rd;
    lens_sample ( p, lens, xy2[2 * i], xy2[2 * i + 1], r4[4 * i], r4[4 * i + 1], r4[4 * i + 2], r4[4 * i + 3], ro, rd );
    float* q = rays8 + 8 * ( size_t ) i;
    q[0] = ro.x; q[1] = ro.y; q[2] = ro.z; q[3] = FLT_MAX;
    q[4] = rd.x; q[5] = rd.y; q[6] = rd.z; q[7] = 0.f;          // (reserved: the all-zero word)
}
hipError_t terra_unit_lens_rays ( const DevRenderParams& p, const DevLens& lens, int n, const uint32_t* xy2, const float* r4, float* rays8 ) {
    if ( n <= 0 ) return hipSuccess;
    hipLaunchKernelGGL ( k_lens_rays, dim3 ( ( n + 255 ) / 256 ), dim3 ( 256 ), 0, 0, p, lens, n, xy2, r4, rays8 );
    return hipGetLastError();
}
#define TERRA_AOV_RAYS_ARG , lens
hipError_t terra_launch_aov_lens ( DevRenderParams p, const DevLens& lens, void* aov, hipStream_t stream ) {
    if ( lens.model < 0 || lens.model > 3 ) return hipErrorInvalidValue;
#elif TERRA_RAY_SOURCE == 1
#define TERRA_AOV_RAYS_ARG , reinterpret_cast<const float4*> ( rays )
hipError_t terra_launch_aov_rays ( DevRenderParams p, const void* rays, void* aov, hipStream_t stream ) {
    if ( !rays ) return hipErrorInvalidValue;
#else
#define TERRA_AOV_RAYS_ARG , mask
hipError_t terra_launch_aov ( DevRenderParams p, void* aov, hipStream_t stream, const uint32_t* mask ) {
#endif
    const uint32_t blocks_x = ( p.w + 15u ) / 16u, blocks_y = ( p.h + 15u ) / 16u;
    const uint64_t vblocks = ( uint64_t ) blocks_x * blocks_y * p.split;
    if ( vblocks == 0 ) return hipSuccess;
    if ( vblocks >= ( 1ull << 32 ) || p.split > 256u || ( 1u << p.split_log2 ) != p.split ) return hipErrorInvalidValue;
    const uint64_t cap = ( uint64_t ) terra_cu_count() * TERRA_AOV_MAX_BLOCKS_PER_CU;
    const uint32_t grid = ( uint32_t ) ( vblocks < cap ? vblocks : cap );
    // the traversal the render call takes (fill_params): the fast tree (MODE 2, or 3 with the reachability replay; its stack as launch_plan.h terra_plan_fast_tree
    // made it) or the reference tree read from global memory (its leaf list: terra_unstaged_leaf_cap) --
    // an LDS-resident scene's reference tree with the leaf-box cull answers with the same closest hit whether it is staged or not, so nothing is staged here
    int mode = 0;
    if ( p.lds_mode == 2 ) { mode = p.scene.reach ? 3 : 2; }
    else { p.stack_depth = p.scene.max_stack < 1 ? 1u : ( uint32_t ) p.scene.max_stack; p.leaf_cap = terra_unstaged_leaf_cap ( p.stack_depth, TERRA_AOV_FOLD_BYTES ); p.spill_cap = 0; }
    const size_t lds = ( size_t ) ( p.stack_depth + ( mode == 0 ? p.leaf_cap : 0u ) ) * 1024 + TERRA_AOV_FOLD_BYTES;
    if ( lds > terra_lds_block_limit() ) return hipErrorInvalidValue;
    const void* fn = mode == 0 ? reinterpret_cast<const void*> ( TERRA_AOV_KERNEL<0> ) : mode == 2 ? reinterpret_cast<const void*> ( TERRA_AOV_KERNEL<2> ) : reinterpret_cast<const void*> ( TERRA_AOV_KERNEL<3> );
    if ( lds > ( size_t ) 64 * 1024 ) { const hipError_t e = hipFuncSetAttribute ( fn, hipFuncAttributeMaxDynamicSharedMemorySize, ( int ) lds ); if ( e != hipSuccess ) return e; }
    uint32_t* spill = nullptr;
    const size_t spill_bytes = mode != 0 ? terra_spill_bytes ( grid, p.spill_cap ) : 0;
    if ( spill_bytes ) { const hipError_t e = hipMallocAsync ( ( void** ) &spill, spill_bytes, stream ); if ( e != hipSuccess ) return e; }
    float4* out = reinterpret_cast<float4*> ( aov );
    if ( mode == 0 ) hipLaunchKernelGGL ( TERRA_AOV_KERNEL<0>, dim3 ( grid ), dim3 ( 256 ), lds, stream, p, out, spill, ( uint32_t ) vblocks, blocks_x TERRA_AOV_RAYS_ARG );
    else if ( mode == 2 ) hipLaunchKernelGGL ( TERRA_AOV_KERNEL<2>, dim3 ( grid ), dim3 ( 256 ), lds, stream, p, out, spill, ( uint32_t ) vblocks, blocks_x TERRA_AOV_RAYS_ARG );
    else hipLaunchKernelGGL ( TERRA_AOV_KERNEL<3>, dim3 ( grid ), dim3 ( 256 ), lds, stream, p, out, spill, ( uint32_t ) vblocks, blocks_x TERRA_AOV_RAYS_ARG );
    const hipError_t e = hipGetLastError();
    if ( spill ) ( void ) hipFreeAsync ( spill, stream );
    return e;
}
