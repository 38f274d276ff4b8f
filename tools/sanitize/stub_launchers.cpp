// sanitizer harness only: host-side stand-ins for this repo's own kernel launchers (no device here)
#include <hip/hip_runtime.h>
#include "kernels.h"
hipError_t terra_launch_render ( const DevRenderParams&, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_render_rays ( const DevRenderParams&, const void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_render_lens ( const DevRenderParams&, const DevLens&, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_render_points ( const DevRenderParams&, const void*, const DevPointSampling&, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_job_streams ( const DevRenderParams&, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_block_order ( const DevRenderParams&, uint32_t*, hipStream_t, const DevLaunchMask*, bool, bool ) { return hipErrorNoDevice; }
hipError_t terra_fill_sincos24 ( float2*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_unit_azimuth24 ( const float2*, float2*, uint32_t* ) { return hipErrorNoDevice; }
hipError_t terra_unit_shade_stages ( int, int, const float*, uint64_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t* ) { return hipErrorNoDevice; }
hipError_t terra_launch_resolve ( const DevRenderParams&, hipStream_t, const uint32_t* ) { return hipErrorNoDevice; }
hipError_t terra_launch_tiles ( bool, float*, void*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, float*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_unit_pcg ( const uint32_t*, int, int, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_stream_keys ( uint64_t, const uint64_t*, const uint64_t*, int, uint64_t* ) { return hipErrorNoDevice; }
hipError_t terra_unit_ray_aabb ( int, const float*, const float*, const float*, int*, float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_watertight ( int, const float*, const float*, const float*, int*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_watertight_pair ( int, const float*, const float*, const float*, int*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_moller_trumbore ( int, const float*, const float*, const float*, int*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_bvh_traverse ( const DevScene&, int, const float*, const float*, int*, uint32_t*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_raycast ( const DevScene&, int, const float*, const float*, int*, int*, float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_trace ( const DevScene&, int, uint32_t, int, const float*, const float*, const uint64_t*, const uint64_t*, float*, uint32_t* ) { return hipErrorNoDevice; }
hipError_t terra_unit_bsdf ( int, int, float*, const float*, const float*, float*, float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_bsdf_at ( int, int, const float*, const float*, const float*, float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_camera ( const DevRenderParams&, int, const uint32_t*, const float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_tonemap ( int, float, int, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_math ( int, int, const float*, const float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_exact_div ( int, const float*, const float*, const float*, uint64_t, uint64_t, float, float, uint64_t, uint32_t*, uint32_t*, unsigned long long*, uint32_t* ) { return hipErrorNoDevice; }
hipError_t terra_unit_exact_sqrt ( int, const float*, const float*, const float*, uint64_t, uint64_t, uint64_t, uint32_t*, uint32_t*, unsigned long long*, uint32_t* ) { return hipErrorNoDevice; }
hipError_t terra_unit_bvh_traverse_fast ( const DevScene&, int, const float*, const float*, int*, uint32_t*, float*, uint32_t* ) { return hipErrorNoDevice; }
hipError_t terra_unit_stratified ( const uint32_t*, int, int, int, int, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_halton ( int, int, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_distribution_1d ( const float*, uint32_t, float*, float*, uint32_t*, const float*, int, float*, float*, uint32_t* ) { return hipErrorNoDevice; }
hipError_t terra_unit_distribution_2d ( const float*, uint32_t, uint32_t, float*, float*, float*, uint32_t*, const float*, int, float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_distribution_2d_pdf ( const float*, uint32_t, uint32_t, float*, float*, float*, uint32_t*, const float*, int, float* ) { return hipErrorNoDevice; }
hipError_t terra_build_fast_tree_device ( const DevTri*, const uint32_t*, uint32_t, float, DevNode*, DevTri*, uint32_t*, int*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_aov ( DevRenderParams, void*, hipStream_t, const uint32_t* ) { return hipErrorNoDevice; }
hipError_t terra_launch_aov_rays ( DevRenderParams, const void*, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_aov_lens ( DevRenderParams, const DevLens&, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_unit_lens_rays ( const DevRenderParams&, const DevLens&, int, const uint32_t*, const float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_launch_aov_points ( DevRenderParams, const void*, const DevPointSampling&, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_unit_point_rays ( const DevPointSampling&, int, const float*, const float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_launch_denoise ( const void*, const void*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int, float, int, float, float*, float*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_moments_accumulate ( const void*, void*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_tile_error ( const void*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, float*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_error_mask ( const float*, uint32_t, uint32_t, uint32_t, float, int, uint32_t*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_denoise_variance ( const void*, const void*, const void*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int, float, int, float, float*, float*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_temporal_reproject ( const DevTemporalParams&, const void*, const void*, const void*, void*, void*, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_query ( DevQueryParams, const void*, size_t, void*, bool, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_nearest ( DevNearestParams, const void*, size_t, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_multi_hit ( DevMultiHitParams, const void*, size_t, uint32_t, void*, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_unit_texture_sample ( const DevTexture*, int, const float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_unit_texture_latlong ( const DevTexture*, int, const float*, float* ) { return hipErrorNoDevice; }
hipError_t terra_launch_atlas_points ( const DevScene&, const DevAtlas&, const float*, void*, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_dilate ( float*, int, int*, uint32_t, uint32_t, int, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_probe_rays ( const void*, uint32_t, uint32_t, const float*, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_sh_project ( const void*, const void*, uint32_t, uint32_t, int, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_sh_irradiance ( const void*, uint32_t, const DevProbeGrid&, const void*, const int*, uint32_t, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_probe_visibility ( const void*, const void*, uint32_t, uint32_t, const DevProbeVisibility&, int, void*, hipStream_t ) { return hipErrorNoDevice; }
hipError_t terra_launch_sh_irradiance_visible ( const void*, const void*, const DevProbeGrid&, const DevProbeVisibility&, const void*, uint32_t, void*, hipStream_t ) { return hipErrorNoDevice; }
