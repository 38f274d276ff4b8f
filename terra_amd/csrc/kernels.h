// kernels.h -- launchers implemented in the .hip files, called by the host side. (How a launch is laid out -- LDS, spill, job scratch, blocks: launch_plan.h.)
#pragma once
#include <hip/hip_runtime.h>
#include "dev_types.h"

hipError_t terra_launch_render ( const DevRenderParams& p, hipStream_t stream );
hipError_t terra_launch_job_streams ( const DevRenderParams& p, hipStream_t stream );      // before terra_launch_render: DevRenderParams::job_streams (none where terra_job_streams_bytes is 0)
// before terra_launch_job_streams: fills p.block_order (= cls + blocks). mask (nullptr: none): a masked launch -- the blocks whose word is zero go last, *mask->live_blocks = the
// blocks before them, p.job_live is set and written whatever `prove`; classify = false: the active blocks are not probed (class 0 all); prove: empty skip (p.job_live set)
hipError_t terra_launch_block_order ( const DevRenderParams& p, uint32_t* cls, hipStream_t stream, const DevLaunchMask* mask, bool classify, bool prove );
// (render_kernels.hip is compiled as several translation units, one per template MODE: 0 reference tree from global memory, 1 LDS-resident, 2 fast tree, 3 fast tree + reachability replay)
hipError_t terra_launch_render_mode0 ( const DevRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_mode1 ( const DevRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_mode2 ( const DevRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_mode3 ( const DevRenderParams& p, size_t lds, hipStream_t stream );
// ray-sourced launches (include/terra_amd.h "Ray-sourced rendering"): terra_launch_render with every primary ray read from rays = one TerraAmdRay per pixel, addressed
// like p.results (st_x / st_y / st_pitch), in place of the camera sample; p without job order and empty skip (block_order, job_live null). The ray-sourced kernel instances
// are units of their own (render_kernels.hip TERRA_TU 4 - 7)
hipError_t terra_launch_render_rays ( const DevRenderParams& p, const void* rays, hipStream_t stream );
hipError_t terra_launch_render_rays_mode0 ( const DevRayRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_rays_mode1 ( const DevRayRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_rays_mode2 ( const DevRayRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_rays_mode3 ( const DevRayRenderParams& p, size_t lds, hipStream_t stream );
// lens launches (include/terra_amd.h "Lens rendering"): terra_launch_render with every primary ray made by lens_sample (trace_geometry.h) from the launch's camera
// fields and `lens`; p without job order and empty skip, as for a ray-sourced launch. The lens kernel instances are units of their own (render_kernels.hip TERRA_TU 8 - 11)
hipError_t terra_launch_render_lens ( const DevRenderParams& p, const DevLens& lens, hipStream_t stream );
hipError_t terra_launch_render_lens_mode0 ( const DevLensRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_lens_mode1 ( const DevLensRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_lens_mode2 ( const DevLensRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_lens_mode3 ( const DevLensRenderParams& p, size_t lds, hipStream_t stream );
// point launches (include/terra_amd.h "Point rendering"): terra_launch_render with every primary ray drawn by point_sample (trace_geometry.h) about the pixel's record
// of `points` (one TerraAmdPoint per pixel, addressed like p.results); p without job order and empty skip, as for a ray-sourced launch. The point kernel instances
// are units of their own (render_kernels.hip TERRA_TU 12 - 15)
hipError_t terra_launch_render_points ( const DevRenderParams& p, const void* points, const DevPointSampling& sampling, hipStream_t stream );
hipError_t terra_launch_render_points_mode0 ( const DevPointRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_points_mode1 ( const DevPointRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_points_mode2 ( const DevPointRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_render_points_mode3 ( const DevPointRenderParams& p, size_t lds, hipStream_t stream );
hipError_t terra_launch_resolve ( const DevRenderParams& p, hipStream_t stream, const uint32_t* live_blocks );   // second kernel of every render; live_blocks: DevLaunchMask::live_blocks of a masked launch, or nullptr
hipError_t terra_launch_tiles ( bool pack, float* pixels, void* results, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                                uint32_t tile, uint32_t rank, uint32_t world, float* packed, hipStream_t stream );

// first-hit AOV pass (aov_kernels.hip): p as fill_params made it, with the render's sample split set (split, split_log2, chunk_spp); aov = TerraAmdAovResult
// per pixel, addressed like p.results (st_x / st_y / st_pitch)
// mask: DevLaunchMask::words of a masked launch (a block whose word is zero is left alone), or nullptr
hipError_t terra_launch_aov ( DevRenderParams p, void* aov, hipStream_t stream, const uint32_t* mask );
// ... with the rays of a ray-sourced launch (as terra_launch_render_rays takes them) in place of the camera's: depth sums |hit point - ray origin|, an inactive ray
// adds its samples and nothing else (aov_kernels.hip compiled as a unit of its own, TERRA_TU 4)
hipError_t terra_launch_aov_rays ( DevRenderParams p, const void* rays, void* aov, hipStream_t stream );
// ... with the samples of a lens launch (as terra_launch_render_lens makes them, the lens pair drawn where that draws it): depth sums |hit point - ray origin|
// (aov_kernels.hip compiled as a unit of its own, TERRA_TU 8)
hipError_t terra_launch_aov_lens ( DevRenderParams p, const DevLens& lens, void* aov, hipStream_t stream );
// ... with the samples of a point launch (as terra_launch_render_points makes them): depth sums |hit point - position|, an inactive point adds its samples and
// nothing else (aov_kernels.hip compiled as a unit of its own, TERRA_TU 12)
hipError_t terra_launch_aov_points ( DevRenderParams p, const void* points, const DevPointSampling& sampling, void* aov, hipStream_t stream );

// the a-trous denoiser and its variance-guided form (denoise_kernels.hip): results / aov / moments (TerraAmdMoments) / radiance / pixels indexed like a frame of fb_w
// pixels per row; only the rectangle is read or written; radiance or pixels may be nullptr
hipError_t terra_launch_denoise ( const void* results, const void* aov, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, int iterations,
                                  float exposure, int op, float gamma, float* radiance, float* pixels, hipStream_t stream );
hipError_t terra_launch_denoise_variance ( const void* results, const void* aov, const void* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, int iterations,
                                           float exposure, int op, float gamma, float* radiance, float* pixels, hipStream_t stream );

// second moments and tile error (variance_kernels.hip): results / moments indexed like a frame of fb_w pixels per row, only the rectangle is read or written;
// errors: one float per tile x tile tile of the rectangle, row-major
hipError_t terra_launch_moments_accumulate ( const void* results, void* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, hipStream_t stream );
hipError_t terra_launch_tile_error ( const void* moments, uint32_t fb_w, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t tile, float* errors, hipStream_t stream );
// the mask of a masked launch over a w x h rectangle from such errors (include/terra_amd.h "Masked rendering"): mask word (bx, by) = all || errors[tile of the block] > target
hipError_t terra_launch_error_mask ( const float* errors, uint32_t w, uint32_t h, uint32_t tile, float target, int all, uint32_t* mask, hipStream_t stream );

// temporal reprojection of a per-pixel history (temporal_kernels.hip; include/terra_amd.h "Temporal reprojection"): every buffer indexed like a frame of fb_w pixels
// per row, only the rectangle is read or written; history_in, out_results, out_moments may be nullptr. cam / prev: the two cameras as fill_camera made them.
struct DevTemporalParams {
    float cam_pos[3], cam_rot[9], tan_half_fov, aspect;
    float prev_pos[3], prev_rot[9], prev_tan_half_fov;
    uint32_t fb_w, fb_h, x, y, w, h;
    float alpha, depth_tolerance, normal_cos, max_length;      // max_length = floor(1 / alpha)
    uint32_t same_camera;                                        // prev_camera equals camera byte for byte
    float inv_fb_w, inv_fb_h;                                    // 1.f / fb_w, 1.f / fb_h as fill_camera rounds them (camera_sample)
};
hipError_t terra_launch_temporal_reproject ( const DevTemporalParams& p, const void* results, const void* aov, const void* history_in, void* history_out,
                                             void* out_results, void* out_moments, hipStream_t stream );

// batched ray queries (query_kernels.hip; include/terra_amd.h "Ray queries"): rays = n TerraAmdRay, out = n TerraAmdHit (closest hit) or n uint32 (anyhit), all in HBM.
// fast: traverse the fast tree (stack_depth / spill_cap as launch_plan.h terra_plan_fast_tree made them; MODE 3 where scene.reach), otherwise the reference tree from global
// memory with stack_depth entries (the launcher plans the leaf list), leaf_cull where the commit proved the cull, for origins within +-origin_limit
struct DevQueryParams {
    DevScene scene;
    uint32_t fast, stack_depth, leaf_cap, spill_cap, leaf_cull;
    float    origin_limit;
};
hipError_t terra_launch_query ( DevQueryParams p, const void* rays, size_t n, void* out, bool anyhit, hipStream_t stream );

// nearest-surface queries (nearest_kernels.hip; include/terra_amd.h "Nearest-surface queries"): queries = n TerraAmdNearestQuery, out = n TerraAmdNearest, both in HBM.
// fast: the distance-ordered walk of the fast tree (stack_depth / spill_cap as launch_plan.h terra_plan_fast_tree made them; scene.fast_nodes_h and at least two
// triangles), otherwise the brute force over scene.tris
struct DevNearestParams {
    DevScene scene;
    uint32_t fast, stack_depth, spill_cap;
};
hipError_t terra_launch_nearest ( DevNearestParams p, const void* queries, size_t n, void* out, hipStream_t stream );

// multi-hit ray queries (multi_hit_kernels.hip; include/terra_amd.h "Multi-hit ray queries"): rays = n TerraAmdRay; k = 1 .. 8: hits = n * k TerraAmdHit, counts = n
// uint32 or nullptr; k = 0: the crossing count, counts = n uint32 and hits is not looked at. All in HBM. fast: the walk of the fast tree (stack_depth / spill_cap as
// launch_plan.h terra_plan_fast_tree made them; MODE 2 and 3 scenes alike), otherwise the brute force over scene.tris
struct DevMultiHitParams {
    DevScene scene;
    uint32_t fast, stack_depth, spill_cap;
};
hipError_t terra_launch_multi_hit ( DevMultiHitParams p, const void* rays, size_t n, uint32_t k, void* hits, void* counts, hipStream_t stream );

// lightmap baking (bake_kernels.hip; include/terra_amd.h "Lightmap baking"): all pointers are device pointers; the launchers take their scratch (the coverage
// keys; the dilation's second copy) from the stream's pool and give it back on the stream
struct DevAtlas {
    uint32_t width, height;
    float    uv_scale[2], uv_offset[2], margin;
};
// points: width * height TerraAmdPoint, texels: width * height TerraAmdAtlasTexel or nullptr; uvs: 6 floats per triangle or nullptr = sc.props' texcoords
hipError_t terra_launch_atlas_points ( const DevScene& sc, const DevAtlas& atlas, const float* uvs, void* points, void* texels, hipStream_t stream );
hipError_t terra_launch_dilate ( float* data, int channels, int* valid, uint32_t width, uint32_t height, int passes, hipStream_t stream );

// probe harmonics (probe_kernels.hip; include/terra_amd.h "Probe harmonics"): all pointers are device pointers, records 16-byte aligned; no scratch, no scene.
// count probes of cells * cells direction cells each (count * cells * cells <= 2^31 - 1)
struct DevProbeGrid {
    int32_t on;                 // 0: index mode (the rest is not looked at)
    int32_t count[3];           // probes along x, y, z
    float   origin[3], spacing[3];
};
// probes: count TerraAmdPoint; jitter: 2 * cells * cells floats or nullptr = cell centres; rays: count * cells * cells TerraAmdRay
hipError_t terra_launch_probe_rays ( const void* probes, uint32_t count, uint32_t cells, const float* jitter, void* rays, hipStream_t stream );
// results: the frame's running sums {float acc[3]; int samples}, rays as above; sh: count TerraAmdProbeSH, read as well where batch > 0
hipError_t terra_launch_sh_project ( const void* results, const void* rays, uint32_t count, uint32_t cells, int batch, void* sh, hipStream_t stream );
// sh: probes TerraAmdProbeSH; points: n TerraAmdPoint; index: n ints (index mode only); out: n float4
hipError_t terra_launch_sh_irradiance ( const void* sh, uint32_t probes, const DevProbeGrid& grid, const void* points, const int* index, uint32_t n, void* out, hipStream_t stream );
// probe visibility (probe_kernels.hip; include/terra_amd.h "Probe visibility"): the options of a call, checked by the host layer (texels 1 .. 16, sharpness 0 .. 8,
// count * texels * texels <= 2^31 - 1)
struct DevProbeVisibility {
    int32_t texels, sharpness;
    float   max_distance, bias;
    int32_t backface;           // flag bit 0
};
// hits: count * cells * cells TerraAmdHit, rays: the TerraAmdRay records they answer; map: count * texels * texels TerraAmdVisibilityTexel, read as well where accumulate != 0
hipError_t terra_launch_probe_visibility ( const void* hits, const void* rays, uint32_t count, uint32_t cells, const DevProbeVisibility& options, int accumulate, void* map, hipStream_t stream );
// sh: TerraAmdProbeSH and map: texels * texels TerraAmdVisibilityTexel for each probe of the grid (grid.on set); points: n TerraAmdPoint; out: n float4
hipError_t terra_launch_sh_irradiance_visible ( const void* sh, const void* map, const DevProbeGrid& grid, const DevProbeVisibility& options, const void* points, uint32_t n, void* out, hipStream_t stream );

hipError_t terra_fill_sincos24 ( float2* table, hipStream_t stream );    // DevScene::sincos24: 2^24 entries (128 MB), device pointer
// table, computed: 2^24 entries each; *mismatches (zeroed by the caller) += the entries of table that tdm_azimuth24 does not reproduce bit for bit
hipError_t terra_unit_azimuth24 ( const float2* table, float2* computed, uint32_t* mismatches );
// the shading stages against the guarded code (unit_kernels.hip "the shading stages"): stage 1 - 3: n rows of 16 floats; staged, guarded: 8 words per row; mask, full_mask:
// a word per row. stage 4: the variate roots, all 2^24; *mismatches (zeroed by the caller) += the offenders; the other pointers are not looked at
hipError_t terra_unit_shade_stages ( int stage, int drops, const float* rows, uint64_t n, uint32_t* staged, uint32_t* guarded, uint32_t* mask, uint32_t* full_mask, uint32_t* mismatches );

// unit-level launchers: all pointers are DEVICE pointers, n items, synchronous semantics left to the caller
hipError_t terra_unit_pcg ( const uint32_t* seeds, int nseeds, int n, float* out );
hipError_t terra_unit_stream_keys ( uint64_t frame_seed, const uint64_t* pix, const uint64_t* k, int n, uint64_t* out3 );
hipError_t terra_unit_ray_aabb ( int n, const float* o, const float* d, const float* boxes, int* hit, float* tmin, float* tmax );
hipError_t terra_unit_watertight ( int n, const float* o, const float* d, const float* tris, int* hit, float* out8 );
hipError_t terra_unit_watertight_pair ( int n, const float* o, const float* d, const float* quads, int* hit, float* depth );
hipError_t terra_unit_moller_trumbore ( int n, const float* o, const float* d, const float* tris, int* hit, float* out4 );
hipError_t terra_unit_bvh_traverse ( const DevScene& sc, int n, const float* o, const float* d, int* found, uint32_t* prim, float* point );
hipError_t terra_unit_bvh_traverse_fast ( const DevScene& sc, int n, const float* o, const float* d, int* found, uint32_t* prim, float* point, uint32_t* nodes_visited );
hipError_t terra_unit_raycast ( const DevScene& sc, int n, const float* o, const float* d, int* obj, int* tri, float* point, float* surface47 );
hipError_t terra_unit_trace ( const DevScene& sc, int integrator, uint32_t bounces, int n, const float* o, const float* d,
                              const uint64_t* stateB, const uint64_t* incB, float* radiance, uint32_t* rand_calls );
hipError_t terra_unit_bsdf ( int kind, int n, float* surfaces47, const float* e3, const float* wo3, float* wi3, float* pdf, float* f3 );
hipError_t terra_unit_bsdf_at ( int kind, int n, const float* surfaces47, const float* wi3, const float* wo3, float* pdf, float* f3 );
hipError_t terra_unit_camera ( const DevRenderParams& p, int n, const uint32_t* xy2, const float* r2, float* dirs3 );
// lens_sample on arrays: r4[n][4] = (r1, r2, l1, l2); rays8[n][8] = TerraAmdRay records (tmax FLT_MAX, reserved 0). p: the camera fields, jitter and frame size
hipError_t terra_unit_lens_rays ( const DevRenderParams& p, const DevLens& lens, int n, const uint32_t* xy2, const float* r4, float* rays8 );
// point_sample on arrays: points8[n][8] = TerraAmdPoint records (device memory, 16-byte aligned), g2[n][2] = (g1, g2); rays8[n][8] = TerraAmdRay records (tmax
// FLT_MAX, reserved 0; all-zero origin and direction for an inactive point)
hipError_t terra_unit_point_rays ( const DevPointSampling& sampling, int n, const float* points8, const float* g2, float* rays8 );
hipError_t terra_unit_tonemap ( int op, float gamma, int n, float* colors3 );
hipError_t terra_unit_math ( int fn, int n, const float* x, const float* y, float* out );
// exact_div.h against "/" (unit_kernels.hip "exact_div.h against the plain"): a == nullptr = the generated set; helper_bits / plain_bits only in the explicit form
hipError_t terra_unit_exact_div ( int op, const float* a, const float* b, const float* c, uint64_t first, uint64_t count, float D, float R, uint64_t seed,
                                  uint32_t* helper_bits, uint32_t* plain_bits, unsigned long long* mismatches, uint32_t* first_bad );
// exact_sqrt.h, make_basis and roulette_scale against their plain forms (unit_kernels.hip "exact_sqrt.h, the one-path"): the same two forms; first_bad[16][21]
hipError_t terra_unit_exact_sqrt ( int op, const float* a, const float* b, const float* c, uint64_t first, uint64_t count, uint64_t seed,
                                   uint32_t* helper_bits, uint32_t* plain_bits, unsigned long long* mismatches, uint32_t* first_bad );
// texture_sample at uv2[n][2] / environment_eval's lat-long lookup at dir3[n][3] on the texture whose descriptor is at `t` (device memory)
hipError_t terra_unit_texture_sample ( const DevTexture* t, int n, const float* uv2, float* out3 );
hipError_t terra_unit_texture_latlong ( const DevTexture* t, int n, const float* dir3, float* out3 );
// SURVEY.md 8f N4 (sampling_device.h): cdf / integrals / monotone are device scratch the caller provides (sizes in scene_host.cpp)
hipError_t terra_unit_stratified ( const uint32_t* seeds, int nseeds, int strata, int samples, int n, float* out2 );
hipError_t terra_unit_halton ( int first, int n, float* out2 );
hipError_t terra_unit_distribution_1d ( const float* f, uint32_t n, float* cdf, float* integral, uint32_t* monotone, const float* e, int m, float* x, float* pdf, uint32_t* idx );
hipError_t terra_unit_distribution_2d ( const float* f, uint32_t nx, uint32_t ny, float* cdf, float* integrals, float* mcdf, uint32_t* monotone, const float* e12, int m, float* xy2, float* pdf );
hipError_t terra_unit_distribution_2d_pdf ( const float* f, uint32_t nx, uint32_t ny, float* cdf, float* integrals, float* mcdf, uint32_t* monotone, const float* xy2, int m, float* pdf );
// the fast tree built on the GPU (tree_build_device.hip): device pointers; out_nodes holds up to n - 1 nodes, out_tris n triangles
// extra_margin: added to the +-1e-4 triangle boxes on every side (0 inside the coordinate range; the rounding bound of the reachability mode outside it)
hipError_t terra_build_fast_tree_device ( const DevTri* tris, const uint32_t* rank, uint32_t n, float extra_margin, DevNode* out_nodes, DevTri* out_tris, uint32_t* n_nodes_out, int* max_stack_out, hipStream_t stream );
