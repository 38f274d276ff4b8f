"""ctypes mirror of the Terra C API (include/Terra.h, include/TerraPresets.h).

Host-side mirror of the reference's client interface for the hot path: the same
type names, field names and entry points as reference include/Terra.h:36-245, so
tests read like a C client of the reference would. One `TerraLib` instance binds
ONE shared library that exports that API:

* the product, ``terra_amd/libterra_amd.so`` (prefix ``terra_``), or
* in tests only, the compiled reference ``oracle/_ref/libterra_ref.so``
  (prefix ``terra_``) and the CPU restatement ``oracle/liboracle.so``
  (prefix ``orc_``).

Nothing here computes anything: it is plumbing over plain pointers and sizes.
"""
from __future__ import annotations

import ctypes as C
from ctypes import POINTER, Structure, c_bool, c_float, c_int, c_size_t, c_uint8, c_uint16, c_uint32, c_uint64, c_void_p

import numpy as np

MAX_ATTRIBUTES = 8

# enum values, reference include/Terra.h:57-69,131-157
kTerraTonemappingOperatorNone, kTerraTonemappingOperatorLinear, kTerraTonemappingOperatorReinhard, \
    kTerraTonemappingOperatorFilmic, kTerraTonemappingOperatorUncharted2 = range(5)
kTerraAcceleratorBVH = 0
kTerraSamplingMethodRandom, kTerraSamplingMethodStratified, kTerraSamplingMethodHalton = range(3)
kTerraIntegratorSimple, kTerraIntegratorDirect, kTerraIntegratorDirectMis, kTerraIntegratorDebugMono, \
    kTerraIntegratorDebugDepth, kTerraIntegratorDebugNormals, kTerraIntegratorDebugMisWeights = range(7)

# preset attribute slots, reference include/TerraPresets.h:11-26
TERRA_DIFFUSE_ALBEDO, TERRA_DIFFUSE_END = 0, 1
TERRA_PHONG_SPECULAR_COLOR, TERRA_PHONG_ALBEDO, TERRA_PHONG_SPECULAR_INTENSITY, TERRA_PHONG_SAMPLE_PICK, TERRA_PHONG_END = 0, 1, 2, 3, 4
TERRA_GGX_F0, TERRA_GGX_ROUGHNESS, TERRA_GGX_END = 0, 1, 2
TERRA_GLASS_TINT, TERRA_GLASS_UNUSED, TERRA_GLASS_SAMPLE_DIR, TERRA_GLASS_SAMPLE_PROB, TERRA_GLASS_END = 0, 1, 2, 3, 4


class TerraFloat2(Structure):
    _fields_ = [("x", c_float), ("y", c_float)]


class TerraFloat3(Structure):
    _fields_ = [("x", c_float), ("y", c_float), ("z", c_float)]

    def __init__(self, x=0.0, y=0.0, z=0.0):
        super().__init__(x, y, z)

    def tuple(self):
        return (self.x, self.y, self.z)


class TerraFloat4(Structure):
    _fields_ = [("x", c_float), ("y", c_float), ("z", c_float), ("w", c_float)]


class TerraFloat4x4(Structure):
    _fields_ = [("rows", TerraFloat4 * 4)]


class TerraShadingSurface(Structure):
    _fields_ = [("transform", TerraFloat4x4), ("normal", TerraFloat3), ("emissive", TerraFloat3),
                ("ior", c_float), ("attributes", TerraFloat3 * MAX_ATTRIBUTES)]


class TerraBSDF(Structure):
    _fields_ = [("sample", c_void_p), ("pdf", c_void_p), ("eval", c_void_p)]


class TerraTexture(Structure):
    _fields_ = [("pixels", c_void_p), ("width", c_uint16), ("height", c_uint16), ("components", c_uint8),
                ("depth", c_uint8), ("filter", c_uint8), ("address_mode", c_uint8)]


class TerraAttribute(Structure):
    _fields_ = [("state", c_void_p), ("finalize", c_void_p), ("eval", c_void_p), ("value", TerraFloat3)]


class TerraMaterial(Structure):
    _fields_ = [("bsdf", TerraBSDF), ("ior", c_float), ("emissive", TerraAttribute),
                ("attributes", TerraAttribute * MAX_ATTRIBUTES), ("attributes_count", c_size_t),
                ("enable_bump_map_attr", c_bool), ("enable_normal_map_attr", c_bool)]


class TerraAABB(Structure):
    _fields_ = [("min", TerraFloat3), ("max", TerraFloat3)]


class TerraTriangle(Structure):
    _fields_ = [("a", TerraFloat3), ("b", TerraFloat3), ("c", TerraFloat3)]


class TerraTriangleProperties(Structure):
    _fields_ = [("normal_a", TerraFloat3), ("normal_b", TerraFloat3), ("normal_c", TerraFloat3),
                ("texcoord_a", TerraFloat2), ("texcoord_b", TerraFloat2), ("texcoord_c", TerraFloat2)]


class TerraObject(Structure):
    _fields_ = [("triangles", POINTER(TerraTriangle)), ("properties", POINTER(TerraTriangleProperties)),
                ("triangles_count", c_size_t), ("material", TerraMaterial)]


class TerraSceneOptions(Structure):
    _fields_ = [("environment_map", TerraAttribute), ("tonemapping_operator", c_int), ("accelerator", c_int),
                ("sampling_method", c_int), ("integrator", c_int), ("subpixel_jitter", c_float),
                ("samples_per_pixel", c_size_t), ("bounces", c_size_t), ("strata", c_size_t),
                ("manual_exposure", c_float), ("gamma", c_float)]


class TerraCamera(Structure):
    _fields_ = [("position", TerraFloat3), ("direction", TerraFloat3), ("up", TerraFloat3), ("fov", c_float)]


class TerraRawIntegrationResult(Structure):
    _fields_ = [("acc", TerraFloat3), ("samples", c_int)]


class TerraFramebuffer(Structure):
    _fields_ = [("pixels", POINTER(TerraFloat3)), ("results", POINTER(TerraRawIntegrationResult)),
                ("width", c_size_t), ("height", c_size_t)]


# sizes pinned by include/Terra.h's TERRA_ABI_ASSERT block
ABI_SIZES = {
    TerraFloat3: 12, TerraFloat4x4: 64, TerraShadingSurface: 188, TerraBSDF: 24, TerraTexture: 16,
    TerraAttribute: 40, TerraMaterial: 408, TerraAABB: 24, TerraTriangle: 36, TerraTriangleProperties: 60,
    TerraObject: 432, TerraSceneOptions: 96, TerraCamera: 40, TerraRawIntegrationResult: 16, TerraFramebuffer: 32,
}
for _t, _s in ABI_SIZES.items():
    assert C.sizeof(_t) == _s, (_t.__name__, C.sizeof(_t), _s)

# numpy views of the array element types
TRIANGLE_DTYPE = np.dtype((np.float32, (3, 3)))          # a, b, c
PROPERTIES_DTYPE = np.dtype((np.float32, (15,)))          # na nb nc (9) + ta tb tc (6)
RESULT_DTYPE = np.dtype([("acc", np.float32, (3,)), ("samples", np.int32)])
assert RESULT_DTYPE.itemsize == 16

# TerraAmdMoments (include/terra_amd.h "Moments buffer"): 32 bytes per pixel
MOMENTS_DTYPE = np.dtype([("seen_acc", np.float32, (3,)), ("seen_samples", np.int32), ("mean", np.float32), ("m2", np.float32), ("batches", np.int32), ("weight", np.int32)])
assert MOMENTS_DTYPE.itemsize == 32


class TerraAmdMoments(Structure):
    _fields_ = [("seen_acc", c_float * 3), ("seen_samples", c_int), ("mean", c_float), ("m2", c_float), ("batches", c_int), ("weight", c_int)]


class TerraAmdAdaptiveOptions(Structure):
    """0 in a field: its default (tile 128, min_batches 4, max_batches 64, target_error 0.05)"""
    _fields_ = [("tile_size", c_size_t), ("min_batches", c_int), ("max_batches", c_int), ("target_error", c_float), ("reserved", c_int)]


class TerraAmdAdaptiveReport(Structure):
    _fields_ = [("rounds", c_int), ("hit_max_batches", c_int), ("tiles", c_int), ("tiles_converged", c_int), ("tile_calls", c_uint64), ("samples", c_uint64),
                ("max_error", c_float), ("reserved", c_int)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


assert C.sizeof(TerraAmdMoments) == 32 and C.sizeof(TerraAmdAdaptiveOptions) == 24 and C.sizeof(TerraAmdAdaptiveReport) == 40

# TerraAmdHistory (include/terra_amd.h "Temporal reprojection"): 48 bytes per pixel
HISTORY_DTYPE = np.dtype([("radiance", np.float32, (3,)), ("length", np.float32), ("normal", np.float32, (3,)), ("depth", np.float32), ("mu1", np.float32), ("mu2", np.float32),
                          ("reserved", np.float32, (2,))])
assert HISTORY_DTYPE.itemsize == 48


class TerraAmdHistory(Structure):
    _fields_ = [("radiance", c_float * 3), ("length", c_float), ("normal", c_float * 3), ("depth", c_float), ("mu1", c_float), ("mu2", c_float), ("reserved", c_float * 2)]


class TerraAmdTemporalOptions(Structure):
    """0 in a field: its default (alpha 0.2, depth_tolerance 0.05, normal_cos 0.9)"""
    _fields_ = [("alpha", c_float), ("depth_tolerance", c_float), ("normal_cos", c_float), ("reserved", c_int)]


assert C.sizeof(TerraAmdHistory) == 48 and C.sizeof(TerraAmdTemporalOptions) == 16

# TerraAmdRay / TerraAmdHit (include/terra_amd.h "Ray queries"): 32 bytes each
RAY_DTYPE = np.dtype([("origin", np.float32, (3,)), ("tmax", np.float32), ("direction", np.float32, (3,)), ("reserved", np.float32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("object", np.int32), ("triangle", np.int32), ("reserved", np.int32), ("point", np.float32, (3,)), ("reserved2", np.float32)])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 32


class TerraAmdRay(Structure):
    _fields_ = [("origin", c_float * 3), ("tmax", c_float), ("direction", c_float * 3), ("reserved", c_float)]


class TerraAmdHit(Structure):
    _fields_ = [("t", c_float), ("object", c_int), ("triangle", c_int), ("reserved", c_int), ("point", c_float * 3), ("reserved2", c_float)]


assert C.sizeof(TerraAmdRay) == 32 and C.sizeof(TerraAmdHit) == 32

# name -> (restype, argtypes) of the ray-query entry points; terra_amd/runtime.py binds them with the rest of the terra_amd_* surface
RAY_QUERY_SIGNATURES = {
    "terra_amd_intersect_device": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "terra_amd_occluded_device": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "terra_amd_intersect": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "terra_amd_occluded": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
}

# ... and of ray-sourced rendering (include/terra_amd.h "Ray-sourced rendering")
RAY_SOURCE_SIGNATURES = {
    "terra_amd_render_rays_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_size_t] * 6 + [c_void_p, c_void_p]),
    "terra_amd_render_rays": (c_int, [c_void_p, c_void_p, POINTER(TerraFramebuffer)] + [c_size_t] * 4),
    "terra_amd_render_aov_rays_device": (c_int, [c_void_p, c_void_p, c_void_p] + [c_size_t] * 6 + [c_void_p]),
    "terra_amd_render_aov_rays": (c_int, [c_void_p, c_void_p, c_void_p] + [c_size_t] * 6),
}

# ... and of masked rendering (include/terra_amd.h "Masked rendering"): the masked camera call, its host and AOV forms, the mask from tile errors, and the adaptive
# driver on masked launches
MASKED_SIGNATURES = {
    "terra_amd_render_masked_device": (c_int, [POINTER(TerraCamera), c_void_p, c_void_p, c_void_p] + [c_size_t] * 6 + [c_void_p, c_void_p, c_void_p]),
    "terra_amd_render_masked": (c_int, [POINTER(TerraCamera), c_void_p, POINTER(TerraFramebuffer)] + [c_size_t] * 4 + [c_void_p]),
    "terra_amd_render_aov_masked_device": (c_int, [POINTER(TerraCamera), c_void_p, c_void_p] + [c_size_t] * 6 + [c_void_p, c_void_p]),
    "terra_amd_error_mask_device": (c_int, [c_void_p, c_size_t, c_size_t, c_size_t, c_float, c_int, c_void_p, c_void_p]),
    "terra_amd_render_adaptive_masked_device": (c_int, [POINTER(TerraCamera), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_size_t] * 6 +
                                                [POINTER(TerraAmdAdaptiveOptions), POINTER(TerraAmdAdaptiveReport), c_void_p]),
    "terra_amd_render_adaptive_masked": (c_int, [POINTER(TerraCamera), c_void_p, POINTER(TerraFramebuffer), c_void_p, c_void_p] + [c_size_t] * 4 +
                                         [POINTER(TerraAmdAdaptiveOptions), POINTER(TerraAmdAdaptiveReport)]),
}



class Lens(Structure):
    """TerraAmdLens (include/terra_amd.h "Lens rendering"): model 0 perspective (pinhole / thin lens), 1 orthographic, 2 equirectangular, 3 fisheye; 32 bytes"""
    _fields_ = [("model", c_int), ("lens_radius", c_float), ("focus_distance", c_float), ("ortho_height", c_float), ("fisheye_fov", c_float), ("reserved", c_int * 3)]


assert C.sizeof(Lens) == 32

# ... and of lens rendering (include/terra_amd.h "Lens rendering")
LENS_SIGNATURES = {
    "terra_amd_render_lens_device": (c_int, [POINTER(TerraCamera), POINTER(Lens), c_void_p, c_void_p, c_void_p] + [c_size_t] * 6 + [c_void_p, c_void_p]),
    "terra_amd_render_lens": (c_int, [POINTER(TerraCamera), POINTER(Lens), c_void_p, POINTER(TerraFramebuffer)] + [c_size_t] * 4),
    "terra_amd_render_aov_lens_device": (c_int, [POINTER(TerraCamera), POINTER(Lens), c_void_p, c_void_p] + [c_size_t] * 6 + [c_void_p]),
    "terra_amd_render_aov_lens": (c_int, [POINTER(TerraCamera), POINTER(Lens), c_void_p, c_void_p] + [c_size_t] * 6),
    "terra_amd_unit_lens_rays": (c_int, [POINTER(TerraCamera), POINTER(Lens), c_size_t, c_size_t, c_int, c_void_p, c_float, c_void_p, c_void_p]),
}

# ... and of the unit entry that holds the short square root, the one-path tangent frame and the roulette rescale to their plain forms (include/terra_amd.h):
# (op, a, b, c, first, count, seed, helper_bits, plain_bits, mismatches, first_bad[16][21])
EXACT_SQRT_SIGNATURES = {
    "terra_amd_unit_exact_sqrt": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]),
}



class Point(Structure):
    """TerraAmdPoint (include/terra_amd.h "Point rendering"): a position and a normal (need not be normalised), one per pixel of a frame; 32 bytes"""
    _fields_ = [("position", c_float * 3), ("reserved", c_float), ("normal", c_float * 3), ("reserved2", c_float)]


class PointSampling(Structure):
    """TerraAmdPointSampling: distribution 0 cosine-weighted hemisphere about the normal, 1 uniform sphere; 16 bytes"""
    _fields_ = [("distribution", c_int), ("reserved", c_int * 3)]


ABI_SIZES.update({Point: 32, PointSampling: 16})
assert C.sizeof(Point) == 32 and C.sizeof(PointSampling) == 16
POINT_DTYPE = np.dtype([("position", np.float32, 3), ("reserved", np.float32), ("normal", np.float32, 3), ("reserved2", np.float32)])
assert POINT_DTYPE.itemsize == 32

# ... and of point rendering (include/terra_amd.h "Point rendering")
POINT_SIGNATURES = {
    "terra_amd_render_points_device": (c_int, [c_void_p, POINTER(PointSampling), c_void_p, c_void_p, c_void_p] + [c_size_t] * 6 + [c_void_p, c_void_p]),
    "terra_amd_render_points": (c_int, [c_void_p, POINTER(PointSampling), c_void_p, POINTER(TerraFramebuffer)] + [c_size_t] * 4),
    "terra_amd_render_aov_points_device": (c_int, [c_void_p, POINTER(PointSampling), c_void_p, c_void_p] + [c_size_t] * 6 + [c_void_p]),
    "terra_amd_render_aov_points": (c_int, [c_void_p, POINTER(PointSampling), c_void_p, c_void_p] + [c_size_t] * 6),
    "terra_amd_unit_point_rays": (c_int, [POINTER(PointSampling), c_int, c_void_p, c_void_p, c_void_p]),
    "terra_amd_scene_vertex_points": (c_int, [c_void_p, c_void_p, c_int]),
}


class Atlas(Structure):
    """TerraAmdAtlas (include/terra_amd.h "Lightmap baking"): the atlas size in texels, uv -> atlas coordinate (uv * uv_scale + uv_offset), the margin in texels; 48 bytes"""
    _fields_ = [("width", c_int), ("height", c_int), ("uv_scale", c_float * 2), ("uv_offset", c_float * 2), ("margin", c_float), ("reserved", c_int * 5)]


class AtlasTexel(Structure):
    """TerraAmdAtlasTexel: the triangle a texel took (-1: uncovered), the weights of its vertices b and c, the squared distance in texels (0 inside); 16 bytes"""
    _fields_ = [("triangle", c_int), ("wb", c_float), ("wc", c_float), ("distance2", c_float)]


ABI_SIZES.update({Atlas: 48, AtlasTexel: 16})
assert C.sizeof(Atlas) == 48 and C.sizeof(AtlasTexel) == 16
ATLAS_TEXEL_DTYPE = np.dtype([("triangle", np.int32), ("wb", np.float32), ("wc", np.float32), ("distance2", np.float32)])
assert ATLAS_TEXEL_DTYPE.itemsize == 16

# ... and of lightmap baking (include/terra_amd.h "Lightmap baking")
BAKE_SIGNATURES = {
    "terra_amd_atlas_points_device": (c_int, [c_void_p, POINTER(Atlas), c_void_p, c_void_p, c_void_p, c_void_p]),
    "terra_amd_atlas_points": (c_int, [c_void_p, POINTER(Atlas), c_void_p, c_void_p, c_void_p]),
    "terra_amd_dilate_device": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "terra_amd_dilate": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int]),
}


class ProbeSH(Structure):
    """TerraAmdProbeSH (include/terra_amd.h "Probe harmonics"): nine real SH coefficients per channel, c[k][channel], and the cells that contributed; 112 bytes"""
    _fields_ = [("c", (c_float * 3) * 9), ("cells", c_int)]


class ProbeGrid(Structure):
    """TerraAmdProbeGrid: nx * ny * nz probes, probe (ix, iy, iz) at origin + i * spacing with the index (iz * ny + iy) * nx + ix; 48 bytes"""
    _fields_ = [("origin", c_float * 3), ("nx", c_int), ("spacing", c_float * 3), ("ny", c_int), ("nz", c_int), ("reserved", c_int * 3)]


ABI_SIZES.update({ProbeSH: 112, ProbeGrid: 48})
assert C.sizeof(ProbeSH) == 112 and C.sizeof(ProbeGrid) == 48
PROBE_SH_DTYPE = np.dtype([("c", np.float32, (9, 3)), ("cells", np.int32)])
assert PROBE_SH_DTYPE.itemsize == 112

# ... and of probe harmonics (include/terra_amd.h "Probe harmonics")
PROBE_SIGNATURES = {
    "terra_amd_probe_rays_device": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_void_p]),
    "terra_amd_probe_rays": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_void_p]),
    "terra_amd_sh_project_device": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p, c_void_p]),
    "terra_amd_sh_project": (c_int, [POINTER(TerraFramebuffer), c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "terra_amd_sh_irradiance_device": (c_int, [c_void_p, c_size_t, POINTER(ProbeGrid), c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "terra_amd_sh_irradiance": (c_int, [c_void_p, c_size_t, POINTER(ProbeGrid), c_void_p, c_void_p, c_size_t, c_void_p]),
    "terra_amd_probe_grid_points": (c_int, [POINTER(ProbeGrid), c_void_p, c_int]),
}


class ProbeVisibility(Structure):
    """TerraAmdProbeVisibility (include/terra_amd.h "Probe visibility"): texels m (1 .. 16) per side of a probe's map, sharpness s (0 .. 8: the weight cos^(2^s)),
    max_distance (a miss, and the cap), bias (the lookup's offset along the normal), flags (bit 0: the lookup's back-face term); 32 bytes"""
    _fields_ = [("texels", c_int), ("sharpness", c_int), ("max_distance", c_float), ("bias", c_float), ("flags", c_int), ("reserved", c_int * 3)]


class VisibilityTexel(Structure):
    """TerraAmdVisibilityTexel: the sums of w, w * d and w * d * d over the cells a texel added, and their number; 16 bytes"""
    _fields_ = [("weight", c_float), ("distance", c_float), ("distance2", c_float), ("cells", c_int)]


PROBE_VISIBILITY_BACKFACE = 1
ABI_SIZES.update({ProbeVisibility: 32, VisibilityTexel: 16})
assert C.sizeof(ProbeVisibility) == 32 and C.sizeof(VisibilityTexel) == 16
VISIBILITY_TEXEL_DTYPE = np.dtype([("weight", np.float32), ("distance", np.float32), ("distance2", np.float32), ("cells", np.int32)])
assert VISIBILITY_TEXEL_DTYPE.itemsize == 16

# ... and of probe visibility (include/terra_amd.h "Probe visibility")
PROBE_VISIBILITY_SIGNATURES = {
    "terra_amd_probe_visibility_device": (c_int, [c_void_p, c_void_p, c_size_t, c_int, POINTER(ProbeVisibility), c_int, c_void_p, c_void_p]),
    "terra_amd_probe_visibility": (c_int, [c_void_p, c_void_p, c_size_t, c_int, POINTER(ProbeVisibility), c_int, c_void_p]),
    "terra_amd_sh_irradiance_visible_device": (c_int, [c_void_p, c_void_p, c_size_t, POINTER(ProbeGrid), POINTER(ProbeVisibility), c_void_p, c_size_t, c_void_p, c_void_p]),
    "terra_amd_sh_irradiance_visible": (c_int, [c_void_p, c_void_p, c_size_t, POINTER(ProbeGrid), POINTER(ProbeVisibility), c_void_p, c_size_t, c_void_p]),
}

# TerraAmdNearestQuery / TerraAmdNearest (include/terra_amd.h "Nearest-surface queries"): 16 and 32 bytes
NEAREST_QUERY_DTYPE = np.dtype([("position", np.float32, (3,)), ("max_distance", np.float32)])
NEAREST_DTYPE = np.dtype([("distance", np.float32), ("object", np.int32), ("triangle", np.uint32), ("feature", np.uint32), ("point", np.float32, (3,)), ("side", np.float32)])
assert NEAREST_QUERY_DTYPE.itemsize == 16 and NEAREST_DTYPE.itemsize == 32


class TerraAmdNearestQuery(Structure):
    _fields_ = [("position", c_float * 3), ("max_distance", c_float)]


class TerraAmdNearest(Structure):
    _fields_ = [("distance", c_float), ("object", c_int), ("triangle", c_uint32), ("feature", c_uint32), ("point", c_float * 3), ("side", c_float)]


ABI_SIZES.update({TerraAmdNearestQuery: 16, TerraAmdNearest: 32})
assert C.sizeof(TerraAmdNearestQuery) == 16 and C.sizeof(TerraAmdNearest) == 32

# ... and of the nearest-surface queries (include/terra_amd.h "Nearest-surface queries")
NEAREST_SIGNATURES = {
    "terra_amd_nearest_device": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "terra_amd_nearest": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "terra_amd_unit_nearest_brute": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
}

# ... and of the multi-hit ray queries (include/terra_amd.h "Multi-hit ray queries"): rays and hits are RAY_DTYPE / HIT_DTYPE records, counts uint32
MAX_HITS = 8
MULTI_HIT_SIGNATURES = {
    "terra_amd_intersect_all_device": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p]),
    "terra_amd_intersect_all": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    "terra_amd_count_hits_device": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "terra_amd_count_hits": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "terra_amd_unit_intersect_all_brute": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    "terra_amd_unit_count_hits_brute": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
}

# entry points of include/Terra.h + include/TerraPresets.h, name -> (restype, argtypes)
API_SIGNATURES = {
    "scene_create": (c_void_p, []),
    "scene_add_object": (POINTER(TerraObject), [c_void_p, c_size_t]),
    "scene_count_objects": (c_size_t, [c_void_p]),
    "scene_commit": (None, [c_void_p]),
    "scene_clear": (None, [c_void_p]),
    "scene_get_options": (POINTER(TerraSceneOptions), [c_void_p]),
    "scene_destroy": (None, [c_void_p]),
    "framebuffer_create": (c_bool, [POINTER(TerraFramebuffer), c_size_t, c_size_t]),
    "framebuffer_clear": (None, [POINTER(TerraFramebuffer)]),
    "framebuffer_destroy": (None, [POINTER(TerraFramebuffer)]),
    "texture_init": (c_bool, [POINTER(TerraTexture), c_size_t, c_size_t, c_size_t, c_void_p]),
    "texture_init_hdr": (c_bool, [POINTER(TerraTexture), c_size_t, c_size_t, c_size_t, c_void_p]),
    "texture_read": (TerraFloat3, [POINTER(TerraTexture), c_size_t, c_size_t]),
    "texture_sample": (TerraFloat3, [c_void_p, c_void_p, c_void_p]),
    "texture_sample_latlong": (TerraFloat3, [c_void_p, c_void_p, c_void_p]),
    "texture_destroy": (None, [POINTER(TerraTexture)]),
    "texture_finalize": (None, [c_void_p]),
    "attribute_init_constant": (None, [POINTER(TerraAttribute), POINTER(TerraFloat3)]),
    "attribute_init_texture": (None, [POINTER(TerraAttribute), POINTER(TerraTexture)]),
    "attribute_init_cubemap": (None, [POINTER(TerraAttribute), POINTER(TerraTexture)]),
    "render": (None, [POINTER(TerraCamera), c_void_p, POINTER(TerraFramebuffer), c_size_t, c_size_t, c_size_t, c_size_t]),
    "malloc": (c_void_p, [c_size_t]),
    "realloc": (c_void_p, [c_void_p, c_size_t]),
    "free": (None, [c_void_p]),
    "log": (None, None),  # variadic
    "bsdf_diffuse_init": (None, [POINTER(TerraBSDF)]),
    "bsdf_phong_init": (None, [POINTER(TerraBSDF)]),
    "bsdf_ggx_init": (None, [POINTER(TerraBSDF)]),
    "bsdf_glass_init": (None, [POINTER(TerraBSDF)]),
}
# not part of the reference API: absent from the compiled reference
OPTIONAL_SYMBOLS = {"bsdf_ggx_init", "bsdf_glass_init"}


class TerraLib:
    """Binds one shared library exporting the Terra.h API under `prefix`."""

    def __init__(self, path: str, prefix: str = "terra_"):
        self.path = str(path)
        self.prefix = prefix
        self.dll = C.CDLL(self.path, mode=getattr(C, "RTLD_LOCAL", 0))
        self.missing = []
        for name, (res, args) in API_SIGNATURES.items():
            sym = prefix + name
            try:
                fn = getattr(self.dll, sym)
            except AttributeError:
                if name not in OPTIONAL_SYMBOLS:
                    self.missing.append(sym)
                continue
            fn.restype = res
            if args is not None:
                fn.argtypes = args
            setattr(self, name, fn)

    def fn(self, symbol: str, restype, argtypes):
        """Bind an extra (non-Terra.h) symbol, e.g. the terra_amd_* or ref_* ones."""
        f = getattr(self.dll, symbol)
        f.restype = restype
        f.argtypes = argtypes
        return f

    def has(self, symbol: str) -> bool:
        try:
            getattr(self.dll, symbol)
            return True
        except AttributeError:
            return False


def f3(v) -> TerraFloat3:
    return TerraFloat3(float(v[0]), float(v[1]), float(v[2]))


def const_attribute(lib: TerraLib, value) -> TerraAttribute:
    a = TerraAttribute()
    v = f3(value)
    lib.attribute_init_constant(C.byref(a), C.byref(v))
    return a


class Framebuffer:
    """Owns a TerraFramebuffer created by `lib` and exposes numpy views of it."""

    def __init__(self, lib: TerraLib, width: int, height: int):
        self.lib = lib
        self.fb = TerraFramebuffer()
        if not lib.framebuffer_create(C.byref(self.fb), width, height):
            raise ValueError("terra_framebuffer_create failed")
        self.width, self.height = width, height

    @property
    def pixels(self) -> np.ndarray:
        n = self.width * self.height
        buf = (c_float * (3 * n)).from_address(C.addressof(self.fb.pixels.contents))
        return np.frombuffer(buf, dtype=np.float32).reshape(self.height, self.width, 3)

    @property
    def results(self) -> np.ndarray:
        n = self.width * self.height
        buf = (C.c_char * (16 * n)).from_address(C.addressof(self.fb.results.contents))
        return np.frombuffer(buf, dtype=RESULT_DTYPE).reshape(self.height, self.width)

    def clear(self):
        self.lib.framebuffer_clear(C.byref(self.fb))

    def destroy(self):
        if self.fb.pixels:
            self.lib.framebuffer_destroy(C.byref(self.fb))
            self.fb.pixels = None
            self.fb.results = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
