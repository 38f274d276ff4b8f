"""Host-side runtime helpers around libterra_amd.so.

PyTorch is used only as plumbing: device memory (framebuffers are torch tensors
whose data_ptr() is handed to the C-ABI), streams and torch.distributed (RCCL).
Import order matters on this image: torch ships its own libamdhip64.so.7, so
torch is imported BEFORE the library is dlopen'ed and the library binds to the
runtime torch already loaded (two HIP runtimes in one process do not see each
other's devices).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

from . import api, scenes

HERE = Path(__file__).resolve().parent
import os as _os
# The number of hardware queues the HIP runtime opens is the host's setting: on shared machines more queues per process than the card has slots is not safe,
# so nothing here raises it (terra_render() callers on several threads still run, their streams share the process's queues).
LIB_PATH = Path(_os.environ.get("TERRA_AMD_LIB", HERE / "libterra_amd.so"))     # TERRA_AMD_LIB: experiment builds (terra_amd/build.py --variant)

_lib: Optional[api.TerraLib] = None


class TerraAmdError(RuntimeError):
    pass


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rays", "nodes", "box_tests", "tri_tests", "hits", "samples", "rand_calls", "attr_fetches", "pixels", "launches", "tri_culled")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class TraversalInfo(C.Structure):
    _fields_ = [("tree_mode", C.c_int), ("fast_tree", C.c_int), ("fast_tree_built_on_device", C.c_int), ("leaf_cull", C.c_int), ("lds_resident", C.c_int), ("max_coordinate", C.c_float), ("max_coordinate_allowed", C.c_float), ("note", C.c_char * 256),
                ("last_call", C.c_int), ("camera_limit", C.c_float)]


CALL_TRAVERSAL = {0: "none", 1: "reference tree, replica traversal", 2: "reference tree + leaf-box cull", 3: "fast tree", 4: "fast tree + reachability replay"}


class SceneInfo(C.Structure):
    _fields_ = [("triangles", C.c_uint32), ("nodes", C.c_uint32), ("objects", C.c_uint32), ("lights", C.c_uint32),
                ("lights_triangles_count", C.c_uint32), ("max_stack", C.c_int32), ("device_bytes", C.c_uint64)]


_CAM = C.POINTER(api.TerraCamera)
_SZ = C.c_size_t
_EXTRA = {
    "terra_amd_last_error": (C.c_char_p, []),
    "terra_amd_clear_error": (None, []),
    "terra_amd_first_error": (C.c_int, [C.c_char_p, C.c_size_t]),
    "terra_amd_clear_first_error": (None, []),
    "terra_amd_thread_staging_bytes": (C.c_size_t, []),
    "terra_amd_device_count": (C.c_int, []),
    "terra_amd_set_device": (C.c_int, [C.c_int]),
    "terra_amd_get_device": (C.c_int, []),
    "terra_amd_set_frame_seed": (None, [C.c_void_p, C.c_uint64]),
    "terra_amd_debug_shrink_reference_boxes": (C.c_int, [C.c_void_p, C.c_float]),
    "terra_amd_debug_pad_stack": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_debug_fast_stack_lds": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_scene_supported": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "terra_amd_init": (C.c_int, []),
    "terra_amd_set_commit_timing": (None, [C.c_int]),
    "terra_amd_set_build_threads": (C.c_int, [C.c_int]),
    "terra_amd_set_azimuth_table": (None, [C.c_int]),
    "terra_amd_get_azimuth_table": (C.c_int, []),
    "terra_amd_azimuth_table_info": (C.c_int, [C.c_void_p]),
    "terra_amd_set_devices": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "terra_amd_get_devices": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "terra_amd_shard_owner": (C.c_int, [C.c_size_t, C.c_int]),
    "terra_amd_render_multi": (C.c_int, [C.POINTER(api.TerraCamera), C.c_void_p, C.POINTER(api.TerraFramebuffer)] + [C.c_size_t] * 5),
    "terra_amd_multi_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "terra_amd_debug_replicas_share_device": (C.c_int, [C.c_int]),
    "terra_amd_set_work_counters": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_work_counters": (C.c_int, [C.c_void_p]),
    "terra_amd_set_sampler_integration": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_sampler_integration": (C.c_int, [C.c_void_p]),
    "terra_amd_set_environment_sampling": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_environment_sampling": (C.c_int, [C.c_void_p]),
    "terra_amd_set_environment_mis": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_environment_mis": (C.c_int, [C.c_void_p]),
    "terra_amd_unit_distribution_2d_pdf": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "terra_amd_unit_azimuth24": (C.c_int, [C.POINTER(C.c_uint32)]),
    "terra_amd_unit_bsdf_at": (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 5),
    "terra_amd_unit_fast_tree": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p]),
    "terra_amd_unit_verify_fast_tree": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t]),
    "terra_amd_get_frame_seed": (C.c_uint64, [C.c_void_p]),
    "terra_amd_set_tree_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_tree_mode": (C.c_int, [C.c_void_p]),
    "terra_amd_traversal_info": (C.c_int, [C.c_void_p, C.POINTER(TraversalInfo)]),
    "terra_amd_set_tree_builder": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_tree_builder": (C.c_int, [C.c_void_p]),
    "terra_amd_set_job_order": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_job_order": (C.c_int, [C.c_void_p]),
    "terra_amd_set_empty_skip": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_empty_skip": (C.c_int, [C.c_void_p]),
    "terra_amd_empty_skip_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "terra_amd_set_leaf_box_test": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_leaf_box_test": (C.c_int, [C.c_void_p]),
    "terra_amd_leaf_box_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "terra_amd_scene_leaf_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "terra_amd_set_leaf_pairs": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_leaf_pairs": (C.c_int, [C.c_void_p]),
    "terra_amd_leaf_pair_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "terra_amd_set_leaf_nearest_first": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_leaf_nearest_first": (C.c_int, [C.c_void_p]),
    "terra_amd_scene_leaf_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "terra_amd_scene_leaf_pair_masks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "terra_amd_leaf_pair_offsets": (C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p]),
    "terra_amd_empty_proof": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float] + [C.c_uint32] * 6 + [C.c_void_p, C.c_size_t]),
    "terra_amd_set_sample_split": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_sample_split": (C.c_int, [C.c_void_p]),
    "terra_amd_auto_sample_split": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_int]),
    "terra_amd_set_environment_lighting": (C.c_int, [C.c_void_p, C.c_int]),
    "terra_amd_get_environment_lighting": (C.c_int, [C.c_void_p]),
    "terra_amd_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "terra_amd_reset_stats": (C.c_int, [C.c_void_p]),
    "terra_amd_scene_info": (C.c_int, [C.c_void_p, C.POINTER(SceneInfo)]),
    "terra_amd_scene_bvh_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "terra_amd_scene_leaf_ranks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "terra_amd_render_device": (C.c_int, [_CAM, C.c_void_p, C.c_void_p, C.c_void_p] + [_SZ] * 6 + [C.c_void_p, C.c_void_p]),
    "terra_amd_render_device_sharded": (C.c_int, [_CAM, C.c_void_p, C.c_void_p, C.c_void_p] + [_SZ] * 7 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "terra_amd_shard_tile_count": (C.c_int, [_SZ, _SZ, _SZ, C.c_int, C.c_int]),
    "terra_amd_shard_packed_bytes": (_SZ, [_SZ, _SZ, _SZ, C.c_int]),
    "terra_amd_pack_tiles": (C.c_int, [C.c_void_p, C.c_void_p] + [_SZ] * 7 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "terra_amd_unpack_tiles": (C.c_int, [C.c_void_p, C.c_void_p] + [_SZ] * 7 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "terra_amd_synchronize": (C.c_int, [C.c_void_p]),
    "terra_amd_time_render_device": (C.c_int, [_CAM, C.c_void_p, C.c_void_p, C.c_void_p] + [_SZ] * 6 + [C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "terra_amd_render_aov_device": (C.c_int, [_CAM, C.c_void_p, C.c_void_p] + [_SZ] * 6 + [C.c_void_p]),
    "terra_amd_render_aov": (C.c_int, [_CAM, C.c_void_p, C.c_void_p] + [_SZ] * 6),
    "terra_amd_denoise_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [_SZ] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "terra_amd_denoise": (C.c_int, [C.c_void_p, C.POINTER(api.TerraFramebuffer), C.c_void_p] + [_SZ] * 4 + [C.c_int, C.c_void_p, C.c_void_p]),
    "terra_amd_accumulate_moments_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [_SZ] * 6 + [C.c_void_p]),
    "terra_amd_accumulate_moments": (C.c_int, [C.c_void_p, C.POINTER(api.TerraFramebuffer), C.c_void_p] + [_SZ] * 4),
    "terra_amd_tile_error_device": (C.c_int, [C.c_void_p, C.c_void_p] + [_SZ] * 7 + [C.c_void_p, C.c_void_p]),
    "terra_amd_tile_error": (C.c_int, [C.POINTER(api.TerraFramebuffer), C.c_void_p] + [_SZ] * 5 + [C.c_void_p]),
    "terra_amd_denoise_variance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [_SZ] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "terra_amd_denoise_variance": (C.c_int, [C.c_void_p, C.POINTER(api.TerraFramebuffer), C.c_void_p, C.c_void_p] + [_SZ] * 4 + [C.c_int, C.c_void_p, C.c_void_p]),
    "terra_amd_render_adaptive_device": (C.c_int, [_CAM, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [_SZ] * 6 +
                                         [C.POINTER(api.TerraAmdAdaptiveOptions), C.POINTER(api.TerraAmdAdaptiveReport), C.c_void_p]),
    "terra_amd_render_adaptive": (C.c_int, [_CAM, C.c_void_p, C.POINTER(api.TerraFramebuffer), C.c_void_p, C.c_void_p] + [_SZ] * 4 +
                                  [C.POINTER(api.TerraAmdAdaptiveOptions), C.POINTER(api.TerraAmdAdaptiveReport)]),
    "terra_amd_reproject_device": (C.c_int, [C.c_void_p, _CAM, _CAM] + [C.c_void_p] * 6 + [_SZ] * 6 + [C.POINTER(api.TerraAmdTemporalOptions), C.c_void_p]),
    "terra_amd_reproject": (C.c_int, [C.c_void_p, _CAM, _CAM, C.POINTER(api.TerraFramebuffer)] + [C.c_void_p] * 5 + [_SZ] * 4 + [C.POINTER(api.TerraAmdTemporalOptions)]),
    **api.RAY_QUERY_SIGNATURES,
    **api.RAY_SOURCE_SIGNATURES,
    **api.MASKED_SIGNATURES,
    **api.LENS_SIGNATURES,
    **api.POINT_SIGNATURES,
    **api.BAKE_SIGNATURES,
    **api.PROBE_SIGNATURES,
    **api.PROBE_VISIBILITY_SIGNATURES,
    **api.EXACT_SQRT_SIGNATURES,
    **api.NEAREST_SIGNATURES,
    **api.MULTI_HIT_SIGNATURES,
}


def load(need_torch: bool = True) -> api.TerraLib:
    """dlopen libterra_amd.so (after torch, see module docstring). Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if need_torch:
        import torch  # noqa: F401  (loads the HIP runtime the library will bind to)
    if not LIB_PATH.exists():
        raise TerraAmdError(f"{LIB_PATH} is missing: run `python -m terra_amd.build` (there is no CPU fallback)")
    lib = api.TerraLib(LIB_PATH, "terra_")
    if lib.missing:
        raise TerraAmdError(f"{LIB_PATH} lacks Terra.h entry points: {lib.missing}")
    for name, (res, args) in _EXTRA.items():
        if lib.has(name):          # (an older build of the library, loaded through TERRA_AMD_LIB for an A/B, lacks the newer entry points: calling one then fails by name)
            setattr(lib, name[len("terra_amd_"):] if name.startswith("terra_amd_") else name, lib.fn(name, res, args))
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> int:
    if rc < 0:
        raise TerraAmdError(f"{what}: {load().last_error().decode()} (status {rc})")
    return rc


def empty_skip_info(lib: api.TerraLib, scene):
    """(proved, total) 16x16 pixel blocks of the scene's most recent launch (terra_amd_empty_skip_info; synchronises the device)"""
    out = (C.c_uint32 * 2)()
    check(lib.empty_skip_info(scene, out), "terra_amd_empty_skip_info")
    return int(out[0]), int(out[1])


def leaf_box_info(lib: api.TerraLib, scene):
    """(used, boxes): whether the scene's most recent launch ran the flat leaf-box test, and the distinct leaf boxes of the committed scene (terra_amd_leaf_box_info)"""
    out = (C.c_uint32 * 2)()
    check(lib.leaf_box_info(scene, out), "terra_amd_leaf_box_info")
    return bool(out[0]), int(out[1])


LEAF_BOX_DTYPE = np.dtype([("min", np.float32, (3,)), ("max", np.float32, (3,)), ("mask", np.uint32)])


def scene_leaf_boxes(lib: api.TerraLib, scene) -> np.ndarray:
    """the committed scene's distinct leaf boxes (terra_amd_scene_leaf_boxes), LEAF_BOX_DTYPE records; needs no device"""
    n = check(lib.scene_leaf_boxes(scene, None, 0), "terra_amd_scene_leaf_boxes")
    out = np.zeros(n, dtype=LEAF_BOX_DTYPE)
    if n:
        check(lib.scene_leaf_boxes(scene, out.ctypes.data, n), "terra_amd_scene_leaf_boxes")
    return out


LEAF_PAIR_DTYPE = np.dtype([("tri", np.uint32, (2,)), ("rank", np.uint32, (2,))])


def leaf_pair_info(lib: api.TerraLib, scene):
    """(used, pairs): whether the scene's most recent launch used the pair form, and the pairs of the committed scene, 0 = no pair form (terra_amd_leaf_pair_info)"""
    out = (C.c_uint32 * 2)()
    check(lib.leaf_pair_info(scene, out), "terra_amd_leaf_pair_info")
    return bool(out[0]), int(out[1])


def scene_leaf_pairs(lib: api.TerraLib, scene):
    """(pairs, masks): the committed scene's pair form (terra_amd_scene_leaf_pairs: LEAF_PAIR_DTYPE records, T1 = (a, b, c) first, ordered by lowest rank; none = no
    pair form) and its distinct leaf boxes' masks in entry bits (terra_amd_scene_leaf_pair_masks); needs no device"""
    n = check(lib.scene_leaf_pairs(scene, None, 0), "terra_amd_scene_leaf_pairs")
    pairs = np.zeros(n, dtype=LEAF_PAIR_DTYPE)
    if n:
        check(lib.scene_leaf_pairs(scene, pairs.ctypes.data, n), "terra_amd_scene_leaf_pairs")
    m = check(lib.scene_leaf_pair_masks(scene, None, 0), "terra_amd_scene_leaf_pair_masks")
    masks = np.zeros(m, dtype=np.uint32)
    if m:
        check(lib.scene_leaf_pair_masks(scene, masks.ctypes.data, m), "terra_amd_scene_leaf_pair_masks")
    return pairs, masks


def leaf_pair_offsets(lib: api.TerraLib, n: int):
    """(entries[6, n], planes[n, 3, 2], section bytes): where a pair launch of n entries stages its LDS section (terra_amd_leaf_pair_offsets)"""
    entries = np.zeros((6, n), dtype=np.uint32)
    planes = np.zeros((n, 3, 2), dtype=np.uint32)
    size = check(lib.leaf_pair_offsets(n, entries.ctypes.data, planes.ctypes.data), "terra_amd_leaf_pair_offsets")
    return entries, planes, size


def last_error() -> str:
    return load().last_error().decode()


def first_error():
    """(status, message) of the first error any thread recorded since the last clear_first_error(); (0, "") if none"""
    buf = C.create_string_buffer(512)
    st = load().first_error(buf, 512)
    return st, buf.value.decode()


class MultiInfo(C.Structure):
    """TerraAmdMultiInfo (include/terra_amd.h)"""
    _fields_ = [("devices", C.c_int), ("device", C.c_int * 16), ("replicas", C.c_int), ("gathers", C.c_uint64), ("last_gather_bytes", C.c_uint64),
                ("process_collectives", C.c_uint64), ("rccl_version", C.c_int), ("communicator_ranks", C.c_int), ("rccl_library", C.c_char * 64), ("rehearsed_gathers", C.c_uint64)]


class DeviceFramebuffer:
    """A TerraFramebuffer that lives in HBM: torch tensors, handed to the C-ABI as raw pointers."""

    def __init__(self, width: int, height: int, device: str = "cuda"):
        import torch
        self.width, self.height = width, height
        self.pixels = torch.zeros(height * width * 3, dtype=torch.float32, device=device)
        self.results = torch.zeros(height * width * 4, dtype=torch.int32, device=device)   # {f32 acc[3]; i32 samples}

    def clear(self):
        self.pixels.zero_(); self.results.zero_()

    def pixels_host(self) -> np.ndarray:
        return self.pixels.cpu().numpy().reshape(self.height, self.width, 3)

    def results_host(self) -> np.ndarray:
        return self.results.cpu().numpy().view(api.RESULT_DTYPE).reshape(self.height, self.width)


def render_device(lib, cam, scene, fb: DeviceFramebuffer, rect: Optional[Tuple[int, int, int, int]] = None, rand_calls=None, stream=None):
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    check(lib.render_device(C.byref(cam), scene, fb.pixels.data_ptr(), fb.results.data_ptr(), fb.width, fb.height, x, y, w, h,
                            rand_calls.data_ptr() if rand_calls is not None else None, stream), "terra_amd_render_device")


class AovResult(C.Structure):
    """TerraAmdAovResult (include/terra_amd.h): running sums of the first hits, 48 bytes"""
    _fields_ = [("albedo", C.c_float * 3), ("coverage", C.c_float), ("normal", C.c_float * 3), ("depth", C.c_float), ("samples", C.c_int), ("reserved", C.c_int * 3)]


AOV_DTYPE = np.dtype([("albedo", np.float32, (3,)), ("coverage", np.float32), ("normal", np.float32, (3,)), ("depth", np.float32), ("samples", np.int32), ("reserved", np.int32, (3,))])
assert AOV_DTYPE.itemsize == C.sizeof(AovResult) == 48


class DeviceAov:
    """A TerraAmdAovResult buffer in HBM (a torch tensor of 12 words per pixel), the companion of a DeviceFramebuffer: clear both together and make
    one render_aov_device call per render call."""

    def __init__(self, width: int, height: int, device: str = "cuda"):
        import torch
        self.width, self.height = width, height
        self.data = torch.zeros(height * width * 12, dtype=torch.int32, device=device)

    def clear(self):
        self.data.zero_()

    def host(self) -> np.ndarray:
        """the raw sums, AOV_DTYPE records (height, width)"""
        return self.data.cpu().numpy().view(AOV_DTYPE).reshape(self.height, self.width)

    def means_host(self):
        """(albedo, normal, depth, coverage): the means over the samples that hit (zero where none did); the normal is the mean vector, not renormalised"""
        a = self.host()
        cov = a["coverage"]
        hit = cov > 0
        div = np.where(hit, cov, np.float32(1))
        albedo = np.where(hit[..., None], a["albedo"] / div[..., None], np.float32(0)).astype(np.float32)
        normal = np.where(hit[..., None], a["normal"] / div[..., None], np.float32(0)).astype(np.float32)
        depth = np.where(hit, a["depth"] / div, np.float32(0)).astype(np.float32)
        return albedo, normal, depth, cov.copy()


def render_aov_device(lib, cam, scene, aov: DeviceAov, rect: Optional[Tuple[int, int, int, int]] = None, stream=None):
    x, y, w, h = rect if rect else (0, 0, aov.width, aov.height)
    check(lib.render_aov_device(C.byref(cam), scene, aov.data.data_ptr(), aov.width, aov.height, x, y, w, h, stream), "terra_amd_render_aov_device")


def denoise_device(lib, scene, fb: DeviceFramebuffer, aov: DeviceAov, iterations: int, rect: Optional[Tuple[int, int, int, int]] = None,
                   radiance=None, pixels=None, stream=None):
    """terra_amd_denoise_device on fb's results and aov's sums; radiance / pixels: float32 tensors of 3 per frame pixel (None: not written;
    pixels may be fb.pixels)"""
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    check(lib.denoise_device(scene, fb.results.data_ptr(), aov.data.data_ptr(), fb.width, fb.height, x, y, w, h, iterations,
                             radiance.data_ptr() if radiance is not None else None, pixels.data_ptr() if pixels is not None else None, stream), "terra_amd_denoise_device")


class DeviceMoments:
    """A TerraAmdMoments buffer in HBM (8 words per pixel), the companion of a DeviceFramebuffer: clear both together and call
    accumulate_moments_device after each render call."""

    def __init__(self, width: int, height: int, device: str = "cuda"):
        import torch
        self.width, self.height = width, height
        self.data = torch.zeros(height * width * 8, dtype=torch.int32, device=device)

    def clear(self):
        self.data.zero_()

    def host(self) -> np.ndarray:
        """api.MOMENTS_DTYPE records (height, width)"""
        return self.data.cpu().numpy().view(api.MOMENTS_DTYPE).reshape(self.height, self.width)

    def variance_host(self) -> np.ndarray:
        """var of each pixel's mean luminance, float32 as the device computes it; -1 where it is unknown (batches < 2)"""
        m = self.host()
        known = m["batches"] >= 2
        den = np.where(known, m["weight"].astype(np.float32) * (m["batches"] - 1).astype(np.float32), np.float32(1))
        return np.where(known, m["m2"] / den, np.float32(-1)).astype(np.float32)


def accumulate_moments_device(lib, scene, fb: DeviceFramebuffer, moments: DeviceMoments, rect: Optional[Tuple[int, int, int, int]] = None, stream=None):
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    check(lib.accumulate_moments_device(scene, fb.results.data_ptr(), moments.data.data_ptr(), fb.width, fb.height, x, y, w, h, stream), "terra_amd_accumulate_moments_device")


def tile_error_device(lib, fb: DeviceFramebuffer, moments: DeviceMoments, tile: int = 0, rect: Optional[Tuple[int, int, int, int]] = None, stream=None):
    """terra_amd_tile_error_device: a float32 tensor of one error per tile of the rectangle, row-major (tile 0: 128)"""
    import torch
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    t = tile or 128
    out = torch.zeros(max(1, -(-w // t) * -(-h // t)), dtype=torch.float32, device=fb.results.device)
    check(lib.tile_error_device(fb.results.data_ptr(), moments.data.data_ptr(), fb.width, fb.height, x, y, w, h, tile, out.data_ptr(), stream), "terra_amd_tile_error_device")
    return out


def denoise_variance_device(lib, scene, fb: DeviceFramebuffer, aov: DeviceAov, moments: DeviceMoments, iterations: int, rect: Optional[Tuple[int, int, int, int]] = None,
                            radiance=None, pixels=None, stream=None):
    """terra_amd_denoise_variance_device; arguments as denoise_device"""
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    check(lib.denoise_variance_device(scene, fb.results.data_ptr(), aov.data.data_ptr(), moments.data.data_ptr(), fb.width, fb.height, x, y, w, h, iterations,
                                      radiance.data_ptr() if radiance is not None else None, pixels.data_ptr() if pixels is not None else None, stream), "terra_amd_denoise_variance_device")


def render_adaptive_device(lib, cam, scene, fb: DeviceFramebuffer, moments: DeviceMoments, aov: Optional[DeviceAov] = None, rect: Optional[Tuple[int, int, int, int]] = None,
                           tile: int = 0, min_batches: int = 0, max_batches: int = 0, target_error: float = 0.0, stream=None, masked: bool = False) -> dict:
    """terra_amd_render_adaptive_device (synchronous); returns the report as a dict. masked: terra_amd_render_adaptive_masked_device -- one masked launch per round
    in place of one call per active tile"""
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    opt = api.TerraAmdAdaptiveOptions(tile, min_batches, max_batches, target_error, 0)
    rep = api.TerraAmdAdaptiveReport()
    fn, what = (lib.render_adaptive_masked_device, "terra_amd_render_adaptive_masked_device") if masked else (lib.render_adaptive_device, "terra_amd_render_adaptive_device")
    check(fn(C.byref(cam), scene, fb.pixels.data_ptr(), fb.results.data_ptr(), moments.data.data_ptr(), aov.data.data_ptr() if aov is not None else None,
             fb.width, fb.height, x, y, w, h, C.byref(opt), C.byref(rep), stream), what)
    return rep.as_dict()


def mask_shape(w: int, h: int) -> Tuple[int, int]:
    """(rows, columns) of the mask of a w x h rectangle: one word per 16 x 16 block (include/terra_amd.h "Masked rendering")"""
    return -(-h // 16), -(-w // 16)


def render_masked_device(lib, cam, scene, fb: DeviceFramebuffer, mask, rect: Optional[Tuple[int, int, int, int]] = None, rand_calls=None, stream=None):
    """terra_amd_render_masked_device; mask: an int32 / uint32 tensor of mask_shape(w, h) words on the framebuffer's device, non-zero = the block is rendered"""
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    rows, cols = mask_shape(w, h)
    if mask.numel() != rows * cols or mask.element_size() != 4:
        raise TerraAmdError(f"mask of {mask.numel()} x {mask.element_size()}-byte words for a {w} x {h} rectangle: {rows * cols} 4-byte words")
    check(lib.render_masked_device(C.byref(cam), scene, fb.pixels.data_ptr(), fb.results.data_ptr(), fb.width, fb.height, x, y, w, h, mask.data_ptr(),
                                   rand_calls.data_ptr() if rand_calls is not None else None, stream), "terra_amd_render_masked_device")


def render_aov_masked_device(lib, cam, scene, aov: DeviceAov, mask, rect: Optional[Tuple[int, int, int, int]] = None, stream=None):
    """terra_amd_render_aov_masked_device; mask as render_masked_device takes it"""
    x, y, w, h = rect if rect else (0, 0, aov.width, aov.height)
    rows, cols = mask_shape(w, h)
    if mask.numel() != rows * cols or mask.element_size() != 4:
        raise TerraAmdError(f"mask of {mask.numel()} x {mask.element_size()}-byte words for a {w} x {h} rectangle: {rows * cols} 4-byte words")
    check(lib.render_aov_masked_device(C.byref(cam), scene, aov.data.data_ptr(), aov.width, aov.height, x, y, w, h, mask.data_ptr(), stream), "terra_amd_render_aov_masked_device")


def error_mask_device(lib, errors, w: int, h: int, tile: int = 0, target_error: float = 0.05, all: bool = False, stream=None):
    """terra_amd_error_mask_device: the int32 mask tensor, mask_shape(w, h), of the blocks whose tile's error (errors: tile_error_device's tensor for the same w, h,
    tile) exceeds target_error -- every block where all"""
    import torch
    rows, cols = mask_shape(w, h)
    out = torch.zeros((rows, cols), dtype=torch.int32, device=errors.device)
    check(lib.error_mask_device(errors.data_ptr(), w, h, tile, target_error, 1 if all else 0, out.data_ptr(), stream), "terra_amd_error_mask_device")
    return out


class DeviceHistory:
    """A TerraAmdHistory buffer in HBM (12 words per pixel). A client keeps two and the previous frame's camera: reproject_device reads one and writes the other,
    then they swap."""

    def __init__(self, width: int, height: int, device: str = "cuda"):
        import torch
        self.width, self.height = width, height
        self.data = torch.zeros(height * width * 12, dtype=torch.float32, device=device)

    def clear(self):
        self.data.zero_()

    def host(self) -> np.ndarray:
        """api.HISTORY_DTYPE records (height, width)"""
        return self.data.cpu().numpy().view(api.HISTORY_DTYPE).reshape(self.height, self.width)


def reproject_device(lib, scene, cam, prev_cam, fb: DeviceFramebuffer, aov: DeviceAov, history_in: Optional[DeviceHistory], history_out: DeviceHistory,
                     out_fb: Optional[DeviceFramebuffer] = None, out_moments: Optional[DeviceMoments] = None, rect: Optional[Tuple[int, int, int, int]] = None,
                     alpha: float = 0.0, depth_tolerance: float = 0.0, normal_cos: float = 0.0, stream=None):
    """terra_amd_reproject_device: blends fb / aov (the current frame under cam) into the history read from history_in (None: the first frame) at the place each
    surface had under prev_cam, and writes history_out; out_fb.results / out_moments receive the blended frame in the form denoise_device /
    denoise_variance_device read (with this frame's aov). 0 in an option: its default."""
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    opt = api.TerraAmdTemporalOptions(alpha, depth_tolerance, normal_cos, 0)
    check(lib.reproject_device(scene, C.byref(cam), C.byref(prev_cam), fb.results.data_ptr(), aov.data.data_ptr(), history_in.data.data_ptr() if history_in is not None else None,
                               history_out.data.data_ptr(), out_fb.results.data_ptr() if out_fb is not None else None, out_moments.data.data_ptr() if out_moments is not None else None,
                               fb.width, fb.height, x, y, w, h, C.byref(opt), stream), "terra_amd_reproject_device")


def _query_rays(rays):
    import torch
    if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8 and rays.is_contiguous()):
        raise TerraAmdError("ray queries take a contiguous float32 tensor [n, 8] on the scene's device: origin, tmax, direction, reserved (api.RAY_DTYPE)")
    return torch, torch.cuda.current_stream(rays.device).cuda_stream or None


def intersect(lib, scene, rays):
    """terra_amd_intersect_device on rays (float32 [n, 8] in HBM: TerraAmdRay records) -> float32 [n, 8], TerraAmdHit records (view the words 1..3 as int32, or
    .cpu().numpy().view(api.HIT_DTYPE)). Queued on the current torch stream; nothing is copied to the host."""
    torch, stream = _query_rays(rays)
    hits = torch.empty((rays.shape[0], 8), dtype=torch.float32, device=rays.device)
    check(lib.intersect_device(scene, rays.data_ptr(), rays.shape[0], hits.data_ptr(), stream), "terra_amd_intersect_device")
    return hits


def occluded(lib, scene, rays):
    """terra_amd_occluded_device on rays (as intersect) -> int32 [n], 1 where something lies within the ray's tmax. Queued on the current torch stream."""
    torch, stream = _query_rays(rays)
    out = torch.empty(rays.shape[0], dtype=torch.int32, device=rays.device)
    check(lib.occluded_device(scene, rays.data_ptr(), rays.shape[0], out.data_ptr(), stream), "terra_amd_occluded_device")
    return out


# ---------------------------------------------------------------------------
# nearest-surface queries (include/terra_amd.h "Nearest-surface queries")
# ---------------------------------------------------------------------------

def nearest(lib, scene, queries):
    """terra_amd_nearest_device on queries (float32 [n, 4] in HBM: TerraAmdNearestQuery records, position and max_distance) -> float32 [n, 8], TerraAmdNearest
    records (.cpu().numpy().view(api.NEAREST_DTYPE)). Queued on the current torch stream; nothing is copied to the host."""
    import torch
    if not (isinstance(queries, torch.Tensor) and queries.is_cuda and queries.dtype == torch.float32 and queries.dim() == 2 and queries.shape[1] == 4 and queries.is_contiguous()):
        raise TerraAmdError("nearest-surface queries take a contiguous float32 tensor [n, 4] on the scene's device: position, max_distance (api.NEAREST_QUERY_DTYPE)")
    if queries.data_ptr() % 16:
        raise TerraAmdError("the query buffer must be 16-byte aligned")
    stream = torch.cuda.current_stream(queries.device).cuda_stream or None
    out = torch.empty((queries.shape[0], 8), dtype=torch.float32, device=queries.device)
    check(lib.nearest_device(scene, queries.data_ptr(), queries.shape[0], out.data_ptr(), stream), "terra_amd_nearest_device")
    return out


def distance_field_points(origin, spacing, dims, max_distance=float("inf")) -> np.ndarray:
    """the queries of distance_field, api.NEAREST_QUERY_DTYPE records [nz, ny, nx]: cell (ix, iy, iz) has its centre at origin + (i + 0.5) * spacing, in float32:
    (float32(i) + 0.5) * spacing, then + origin"""
    nx, ny, nz = (int(v) for v in dims)
    if nx < 1 or ny < 1 or nz < 1:
        raise TerraAmdError(f"distance_field: dims {dims} must be positive")
    o = np.asarray(origin, np.float32).reshape(3)
    s = np.broadcast_to(np.asarray(spacing, np.float32), (3,))
    q = np.zeros((nz, ny, nx), api.NEAREST_QUERY_DTYPE)
    axes = [(np.arange(n, dtype=np.float32) + np.float32(0.5)) * s[a] + o[a] for a, n in enumerate((nx, ny, nz))]
    q["position"][..., 0] = axes[0][None, None, :]
    q["position"][..., 1] = axes[1][None, :, None]
    q["position"][..., 2] = axes[2][:, None, None]
    q["max_distance"] = np.float32(max_distance)
    return q


def distance_field(lib, scene, origin, spacing, dims, max_distance=float("inf"), signed=False):
    """The scene's distance field on a regular grid -> float32 [nz, ny, nx] in HBM: the `distance` of nearest() at the cell centres of distance_field_points
    (FLT_MAX where nothing lies within max_distance). signed=True: the distance times `side` where the closest feature is a face (feature == 0), left positive at
    edges and vertices -- a CRUDE sign: it follows the winning triangle's winding, says nothing true next to an edge or a vertex, and is no inside / outside test of
    an open or inconsistently wound scene (angle-weighted pseudonormals are not built). signed="crossings": the distance negated where inside() says 1 -- the
    crossing-count sign, which needs a closed surface and no winding."""
    import torch
    q = distance_field_points(origin, spacing, dims, max_distance)
    queries = torch.from_numpy(q.view(np.float32).reshape(-1, 4)).cuda()
    out = nearest(lib, scene, queries)
    dist = out[:, 0]
    if isinstance(signed, str):
        if signed != "crossings":
            raise TerraAmdError(f"distance_field: signed={signed!r}; False, True or \"crossings\"")
        dist = torch.where(inside(lib, scene, queries[:, :3].contiguous()) == 1, -dist, dist)
    elif signed:
        feature = out[:, 3].view(torch.int32)
        side = out[:, 7]
        dist = torch.where((feature == 0) & (side != 0), dist * side, dist)
    return dist.reshape(q.shape).contiguous()


# ---------------------------------------------------------------------------
# multi-hit ray queries (include/terra_amd.h "Multi-hit ray queries")
# ---------------------------------------------------------------------------

def intersect_all(lib, scene, rays, k):
    """terra_amd_intersect_all_device on rays (float32 [n, 8] in HBM: TerraAmdRay records) -> (hits float32 [n, k, 8]: per ray its first k hits by (depth, rank) as
    TerraAmdHit records, miss records after the last; counts int32 [n]: the hit records written). 1 <= k <= api.MAX_HITS. Queued on the current torch stream;
    nothing is copied to the host."""
    torch, stream = _query_rays(rays)
    k = int(k)
    if not 1 <= k <= api.MAX_HITS:
        raise TerraAmdError(f"intersect_all: k = {k}, 1 to {api.MAX_HITS}")
    n = rays.shape[0]
    hits = torch.empty((n, k, 8), dtype=torch.float32, device=rays.device)
    counts = torch.empty(n, dtype=torch.int32, device=rays.device)
    check(lib.intersect_all_device(scene, rays.data_ptr(), n, k, hits.data_ptr(), counts.data_ptr(), stream), "terra_amd_intersect_all_device")
    return hits, counts


def count_hits(lib, scene, rays):
    """terra_amd_count_hits_device on rays (as intersect) -> int32 [n]: how many triangles each ray crosses within its tmax. Queued on the current torch stream."""
    torch, stream = _query_rays(rays)
    out = torch.empty(rays.shape[0], dtype=torch.int32, device=rays.device)
    check(lib.count_hits_device(scene, rays.data_ptr(), rays.shape[0], out.data_ptr(), stream), "terra_amd_count_hits_device")
    return out


# the three directions of inside(), used as float32: cyclic shifts of (0.48, 0.64, 0.60) with one sign turned, of unit length (48^2 + 64^2 + 60^2 = 100^2), none
# along an axis or a diagonal of the usual modelling grids
INSIDE_DIRECTIONS = ((0.48, 0.64, 0.60), (-0.60, 0.48, 0.64), (0.64, -0.60, 0.48))


def inside(lib, scene, points):
    """Which points (float32 [n, 3] in HBM) lie inside the scene's closed surfaces -> int32 [n], 1 = inside: three rays to infinity per point along
    INSIDE_DIRECTIONS, count_hits on each, 1 where at least two of the three counts are odd (one ray through a shared edge or vertex may count both neighbours;
    two of three doing so is what the vote leaves). Needs a closed surface; an open mesh has no inside. Queued on the current torch stream."""
    import torch
    if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 3):
        raise TerraAmdError("inside takes a float32 tensor [n, 3] on the scene's device")
    n = points.shape[0]
    rays = torch.zeros((3, n, 8), dtype=torch.float32, device=points.device)
    rays[:, :, 0:3] = points[None, :, :]
    rays[:, :, 3] = float("inf")
    rays[:, :, 4:7] = torch.tensor(INSIDE_DIRECTIONS, dtype=torch.float32, device=points.device)[:, None, :]
    odd = count_hits(lib, scene, rays.reshape(3 * n, 8)).reshape(3, n) & 1
    return (odd.sum(dim=0) >= 2).to(torch.int32)


def probe_clearance(lib, scene, probes):
    """How far each probe is from the scene's surfaces: probes (float32 [n, 8] in HBM, api.POINT_DTYPE records; only the position is read) -> (distance float32 [n],
    closest point float32 [n, 3]) in HBM -- what a client needs to drop or move the probes of a grid that landed inside or next to a wall."""
    import torch
    if not (isinstance(probes, torch.Tensor) and probes.is_cuda and probes.dtype == torch.float32 and probes.dim() == 2 and probes.shape[1] == 8):
        raise TerraAmdError("probe_clearance takes a float32 tensor [n, 8] on the scene's device: api.POINT_DTYPE records")
    q = torch.empty((probes.shape[0], 4), dtype=torch.float32, device=probes.device)
    q[:, :3] = probes[:, :3]
    q[:, 3] = float("inf")
    out = nearest(lib, scene, q)
    return out[:, 0].contiguous(), out[:, 4:7].contiguous()


# ---------------------------------------------------------------------------
# ray-sourced rendering (include/terra_amd.h "Ray-sourced rendering")
# ---------------------------------------------------------------------------

def _frame_rays(rays, width: int, height: int):
    import torch
    if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32 and rays.is_contiguous() and tuple(rays.shape) == (height, width, 8)):
        raise TerraAmdError(f"ray-sourced calls take a contiguous float32 tensor [{height}, {width}, 8] on the scene's device: one api.RAY_DTYPE record per pixel of the frame")
    if rays.data_ptr() % 16:
        raise TerraAmdError("the ray buffer must be 16-byte aligned")


def render_rays_device(lib, scene, rays, fb: DeviceFramebuffer, rect: Optional[Tuple[int, int, int, int]] = None, rand_calls=None, stream=None):
    """terra_amd_render_rays_device: the render call with every pixel's primary ray read from rays (float32 [fb.height, fb.width, 8] in HBM: TerraAmdRay records)"""
    _frame_rays(rays, fb.width, fb.height)
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    check(lib.render_rays_device(scene, rays.data_ptr(), fb.pixels.data_ptr(), fb.results.data_ptr(), fb.width, fb.height, x, y, w, h,
                                 rand_calls.data_ptr() if rand_calls is not None else None, stream), "terra_amd_render_rays_device")


def render_aov_rays_device(lib, scene, rays, aov: DeviceAov, rect: Optional[Tuple[int, int, int, int]] = None, stream=None):
    """terra_amd_render_aov_rays_device: the AOV pass of a render_rays_device call (rays as there)"""
    _frame_rays(rays, aov.width, aov.height)
    x, y, w, h = rect if rect else (0, 0, aov.width, aov.height)
    check(lib.render_aov_rays_device(scene, rays.data_ptr(), aov.data.data_ptr(), aov.width, aov.height, x, y, w, h, stream), "terra_amd_render_aov_rays_device")


# ---------------------------------------------------------------------------
# lens rendering (include/terra_amd.h "Lens rendering")
# ---------------------------------------------------------------------------

def render_lens_device(lib, cam, lens: api.Lens, scene, fb: DeviceFramebuffer, rect: Optional[Tuple[int, int, int, int]] = None, rand_calls=None, stream=None):
    """terra_amd_render_lens_device: the render call with every sample's primary ray made from the camera model `lens`"""
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    check(lib.render_lens_device(C.byref(cam), C.byref(lens), scene, fb.pixels.data_ptr(), fb.results.data_ptr(), fb.width, fb.height, x, y, w, h,
                                 rand_calls.data_ptr() if rand_calls is not None else None, stream), "terra_amd_render_lens_device")


def render_aov_lens_device(lib, cam, lens: api.Lens, scene, aov: DeviceAov, rect: Optional[Tuple[int, int, int, int]] = None, stream=None):
    """terra_amd_render_aov_lens_device: the AOV pass of a render_lens_device call"""
    x, y, w, h = rect if rect else (0, 0, aov.width, aov.height)
    check(lib.render_aov_lens_device(C.byref(cam), C.byref(lens), scene, aov.data.data_ptr(), aov.width, aov.height, x, y, w, h, stream), "terra_amd_render_aov_lens_device")


def lens_rays(lib, cam, lens: api.Lens, width: int, height: int, xy, jitter: float, r4) -> np.ndarray:
    """terra_amd_unit_lens_rays: the device's ray generator on arrays. xy [n, 2] pixels of a width x height frame, r4 [n, 4] = (r1, r2, l1, l2);
    returns n api.RAY_DTYPE records (tmax FLT_MAX, reserved 0), which the ray door takes as they are"""
    xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
    r4 = np.ascontiguousarray(r4, dtype=np.float32).reshape(-1, 4)
    if len(xy) != len(r4):
        raise TerraAmdError("lens_rays: one (r1, r2, l1, l2) per pixel")
    out = np.zeros(len(xy), dtype=api.RAY_DTYPE)
    check(lib.unit_lens_rays(C.byref(cam), C.byref(lens), width, height, len(xy), xy.ctypes.data, jitter, r4.ctypes.data, out.ctypes.data), "terra_amd_unit_lens_rays")
    return out


RADIANCE_FRAME_WIDTH = 256


def radiance_frame_shape(n: int) -> Tuple[int, int]:
    """(height, width) of the frame radiance() folds n rays into: rows of RADIANCE_FRAME_WIDTH pixels, the last one padded"""
    return max(1, -(-n // RADIANCE_FRAME_WIDTH)), RADIANCE_FRAME_WIDTH


def fold_rays(rays, xp=np):
    """n ray records [n, 8] -> a frame [height, 256, 8] (radiance_frame_shape), ray i at pixel (i % 256, i // 256), padded with inactive records (all zero:
    a zero direction). A pure function of its input: xp is numpy, or torch for a tensor (which stays on its device)."""
    n = int(rays.shape[0])
    h, w = radiance_frame_shape(n)
    if xp is np:
        frame = np.zeros((h * w, 8), dtype=np.float32)
    else:
        frame = xp.zeros((h * w, 8), dtype=xp.float32, device=rays.device)
    frame[:n] = rays
    return frame.reshape(h, w, 8)


def unfold_pixels(frame, n: int):
    """the first n pixels of a folded frame [height, 256, k], in the rays' order: [n, k]"""
    return frame.reshape(-1, frame.shape[-1])[:n]


def radiance(lib, scene, rays, batches: int = 1):
    """Mean radiance along n rays (float32 [n, 8] in HBM: TerraAmdRay records) -> float32 [n, 3]: the rays folded into a frame 256 pixels wide, `batches`
    render_rays_device calls of the scene's samples_per_pixel each, acc / samples (NaN-free: an inactive ray's mean is 0). Queued on the current torch stream;
    nothing goes through the host."""
    torch, stream = _query_rays(rays)
    if batches < 1:
        raise TerraAmdError("radiance: batches must be at least 1")
    n = rays.shape[0]
    frame = fold_rays(rays, torch)
    h, w = frame.shape[0], frame.shape[1]
    with torch.cuda.device(rays.device):
        fb = DeviceFramebuffer(w, h, device=rays.device)
        for _ in range(batches):
            render_rays_device(lib, scene, frame, fb, stream=stream)
        res = fb.results.view(h, w, 4)
        acc = res[..., :3].view(torch.float32)
        samples = res[..., 3:4].to(torch.float32)
        return unfold_pixels(acc / samples, n).contiguous()


# ---------------------------------------------------------------------------
# point rendering (include/terra_amd.h "Point rendering")
# ---------------------------------------------------------------------------

def point_sampling(distribution: int = 0) -> api.PointSampling:
    """api.PointSampling with `distribution` (0 cosine-weighted hemisphere about the normal, 1 uniform sphere)"""
    ps = api.PointSampling()
    ps.distribution = distribution
    return ps


def _frame_points(points, width: int, height: int):
    import torch
    if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float32 and points.is_contiguous() and tuple(points.shape) == (height, width, 8)):
        raise TerraAmdError(f"point calls take a contiguous float32 tensor [{height}, {width}, 8] on the scene's device: one api.POINT_DTYPE record per pixel of the frame")
    if points.data_ptr() % 16:
        raise TerraAmdError("the point buffer must be 16-byte aligned")


def render_points_device(lib, scene, sampling: api.PointSampling, points, fb: DeviceFramebuffer, rect: Optional[Tuple[int, int, int, int]] = None, rand_calls=None, stream=None):
    """terra_amd_render_points_device: the render call with every sample's primary ray drawn about the pixel's point (float32 [fb.height, fb.width, 8] in HBM:
    TerraAmdPoint records)"""
    _frame_points(points, fb.width, fb.height)
    x, y, w, h = rect if rect else (0, 0, fb.width, fb.height)
    check(lib.render_points_device(scene, C.byref(sampling), points.data_ptr(), fb.pixels.data_ptr(), fb.results.data_ptr(), fb.width, fb.height, x, y, w, h,
                                   rand_calls.data_ptr() if rand_calls is not None else None, stream), "terra_amd_render_points_device")


def render_aov_points_device(lib, scene, sampling: api.PointSampling, points, aov: DeviceAov, rect: Optional[Tuple[int, int, int, int]] = None, stream=None):
    """terra_amd_render_aov_points_device: the AOV pass of a render_points_device call (points as there); with distribution 0, 1 - coverage / samples is ambient occlusion"""
    _frame_points(points, aov.width, aov.height)
    x, y, w, h = rect if rect else (0, 0, aov.width, aov.height)
    check(lib.render_aov_points_device(scene, C.byref(sampling), points.data_ptr(), aov.data.data_ptr(), aov.width, aov.height, x, y, w, h, stream), "terra_amd_render_aov_points_device")


def point_rays(lib, sampling: api.PointSampling, points, g2) -> np.ndarray:
    """terra_amd_unit_point_rays: the device's generator on arrays. points: n api.POINT_DTYPE records (or float32 [n, 8]), g2 [n, 2] = (g1, g2); returns n
    api.RAY_DTYPE records (tmax FLT_MAX, reserved 0; all zero for an inactive point), which the ray door takes as they are"""
    pts = np.ascontiguousarray(points)
    pts = np.ascontiguousarray(pts.view(np.float32) if pts.dtype == api.POINT_DTYPE else pts.astype(np.float32, copy=False)).reshape(-1, 8)
    g2 = np.ascontiguousarray(g2, dtype=np.float32).reshape(-1, 2)
    if len(pts) != len(g2):
        raise TerraAmdError("point_rays: one (g1, g2) per point")
    out = np.zeros(len(pts), dtype=api.RAY_DTYPE)
    check(lib.unit_point_rays(C.byref(sampling), len(pts), pts.ctypes.data, g2.ctypes.data, out.ctypes.data), "terra_amd_unit_point_rays")
    return out


def scene_vertex_points(lib, scene) -> np.ndarray:
    """terra_amd_scene_vertex_points: the committed scene's vertices as api.POINT_DTYPE records, record 3 T + k = vertex k of triangle T with its stored normal"""
    n = check(lib.scene_vertex_points(scene, None, 0), "terra_amd_scene_vertex_points")
    out = np.zeros(n, dtype=api.POINT_DTYPE)
    if n:
        check(lib.scene_vertex_points(scene, out.ctypes.data, n), "terra_amd_scene_vertex_points")
    return out


def fold_points(positions, normals, xp=np):
    """n points ([n, 3] positions, [n, 3] normals) -> a frame [height, 256, 8] of TerraAmdPoint records (radiance_frame_shape), point i at pixel (i % 256, i // 256),
    padded with inactive points (all zero: a zero normal). xp is numpy, or torch for tensors (which stay on their device)."""
    n = int(positions.shape[0])
    h, w = radiance_frame_shape(n)
    if xp is np:
        frame = np.zeros((h * w, 8), dtype=np.float32)
    else:
        frame = xp.zeros((h * w, 8), dtype=xp.float32, device=positions.device)
    frame[:n, 0:3] = positions
    frame[:n, 4:7] = normals
    return frame.reshape(h, w, 8)


def irradiance(lib, scene, positions, normals, spp_batches: int = 1, distribution: int = 0):
    """Irradiance at n points (float32 [n, 3] positions and normals in HBM) -> float32 [n, 3]: the points folded into a frame 256 pixels wide, `spp_batches`
    render_points_device calls of the scene's samples_per_pixel each, PI * acc / samples (an inactive point's is 0). With distribution 1 the same factor is applied to
    the probe's mean radiance over the sphere. Queued on the current torch stream; nothing goes through the host."""
    import math
    import torch
    for t in (positions, normals):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3):
            raise TerraAmdError("irradiance takes float32 tensors [n, 3] on the scene's device: the points' positions and normals")
    if positions.shape[0] != normals.shape[0] or positions.device != normals.device:
        raise TerraAmdError("irradiance: one normal per position, on the same device")
    stream = torch.cuda.current_stream(positions.device).cuda_stream or None
    if spp_batches < 1:
        raise TerraAmdError("irradiance: spp_batches must be at least 1")
    n = positions.shape[0]
    frame = fold_points(positions, normals, torch)
    h, w = frame.shape[0], frame.shape[1]
    ps = point_sampling(distribution)
    with torch.cuda.device(positions.device):
        fb = DeviceFramebuffer(w, h, device=positions.device)
        for _ in range(spp_batches):
            render_points_device(lib, scene, ps, frame, fb, stream=stream)
        res = fb.results.view(h, w, 4)
        acc = res[..., :3].view(torch.float32)
        samples = res[..., 3:4].to(torch.float32)
        return unfold_pixels(acc / samples * math.pi, n).contiguous()


# ---------------------------------------------------------------------------
# lightmap baking (include/terra_amd.h "Lightmap baking")
# ---------------------------------------------------------------------------

def atlas_of(width: int, height: int, uv_scale=None, uv_offset=None, margin: float = 0.5) -> api.Atlas:
    """api.Atlas of width x height texels; uv_scale / uv_offset (pairs) default to (1, 1) / (0, 0): uvs already in texels"""
    a = api.Atlas()
    a.width, a.height, a.margin = width, height, margin
    a.uv_scale[:] = (1.0, 1.0) if uv_scale is None else tuple(uv_scale)
    a.uv_offset[:] = (0.0, 0.0) if uv_offset is None else tuple(uv_offset)
    return a


def _current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream or None


def atlas_points(lib, scene, atlas: api.Atlas, uvs=None):
    """terra_amd_atlas_points_device on the current torch stream: (points, texels) in HBM -- points float32 [height, width, 8], the api.POINT_DTYPE records
    render_points_device takes as they are; texels int32 [height, width, 4], api.ATLAS_TEXEL_DTYPE records (triangle, then the bits of wb, wc, distance2).
    uvs: float32 [triangles, 6] (ua va ub vb uc vc) in HBM, or None = the scene's own texcoords."""
    import torch
    if uvs is not None and not (isinstance(uvs, torch.Tensor) and uvs.is_cuda and uvs.dtype == torch.float32 and uvs.is_contiguous() and uvs.dim() == 2 and uvs.shape[1] == 6):
        raise TerraAmdError("atlas_points takes uvs as a contiguous float32 tensor [triangles, 6] on the scene's device")
    points = torch.empty((atlas.height, atlas.width, 8), dtype=torch.float32, device="cuda")
    texels = torch.empty((atlas.height, atlas.width, 4), dtype=torch.int32, device="cuda")
    check(lib.atlas_points_device(scene, C.byref(atlas), uvs.data_ptr() if uvs is not None else None, points.data_ptr(), texels.data_ptr(), _current_stream()),
          "terra_amd_atlas_points_device")
    return points, texels


def dilate(data, valid, passes: int):
    """terra_amd_dilate_device in place on the current torch stream: data float32 [height, width, channels] (or [height, width]), valid int32 [height, width], in HBM"""
    import torch
    if not (isinstance(data, torch.Tensor) and data.is_cuda and data.dtype == torch.float32 and data.is_contiguous() and data.dim() in (2, 3)):
        raise TerraAmdError("dilate takes data as a contiguous float32 tensor [height, width, channels] in HBM")
    h, w = int(data.shape[0]), int(data.shape[1])
    if not (isinstance(valid, torch.Tensor) and valid.is_cuda and valid.dtype == torch.int32 and valid.is_contiguous() and tuple(valid.shape) == (h, w)):
        raise TerraAmdError(f"dilate takes valid as a contiguous int32 tensor [{h}, {w}] in HBM")
    check(load().dilate_device(data.data_ptr(), int(data.shape[2]) if data.dim() == 3 else 1, valid.data_ptr(), w, h, passes, _current_stream()), "terra_amd_dilate_device")


_dilate = dilate          # (bake_lightmap's `dilate` argument is the pass count)


def bake_lightmap(lib, scene, width: int, height: int, uvs=None, uv_scale=None, margin: float = 0.5, dilate: int = 2, batches: int = 1):
    """A lightmap of the committed scene -> (irradiance float32 [height, width, 3], texels as atlas_points returns them), in HBM: atlas_points ->
    `batches` render_points_device calls (distribution 0) of the scene's samples_per_pixel each -> PI * acc / samples -> `dilate` passes of dilation with
    triangle >= 0 as the validity (an uncovered texel that no pass reaches stays 0). Everything is queued on the current torch stream."""
    import math
    import torch
    if batches < 1:
        raise TerraAmdError("bake_lightmap: batches must be at least 1")
    points, texels = atlas_points(lib, scene, atlas_of(width, height, uv_scale=uv_scale, margin=margin), uvs)
    fb = DeviceFramebuffer(width, height)
    ps = point_sampling(0)
    stream = _current_stream()
    for _ in range(batches):
        render_points_device(lib, scene, ps, points, fb, stream=stream)
    res = fb.results.view(height, width, 4)
    irradiance = (math.pi * res[..., :3].view(torch.float32) / res[..., 3:4].to(torch.float32)).contiguous()
    valid = (texels[..., 0] >= 0).to(torch.int32).contiguous()
    _dilate(irradiance, valid, dilate)
    return irradiance, texels


# ---------------------------------------------------------------------------
# probe harmonics (include/terra_amd.h "Probe harmonics")
# ---------------------------------------------------------------------------

def _records(t, words: int, what: str):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.float32, torch.int32) and t.is_contiguous() and t.numel() % words == 0):
        raise TerraAmdError(f"{what}: a contiguous float32 or int32 tensor of {words} words per record in HBM")
    if t.data_ptr() % 16:
        raise TerraAmdError(f"{what}: the buffer must be 16-byte aligned")
    return t.numel() // words


def probe_grid(lib, origin, spacing, counts):
    """(api.ProbeGrid, points): the grid of counts = (nx, ny, nz) probes, probe (ix, iy, iz) at origin + i * spacing, and its probes as api.POINT_DTYPE records in
    index order with the normal (0, 0, 1) (terra_amd_probe_grid_points; needs no device)"""
    g = api.ProbeGrid()
    g.origin[:] = tuple(origin)
    g.spacing[:] = tuple(spacing)
    g.nx, g.ny, g.nz = (int(c) for c in counts)
    n = check(lib.probe_grid_points(C.byref(g), None, 0), "terra_amd_probe_grid_points")
    points = np.zeros(n, dtype=api.POINT_DTYPE)
    check(lib.probe_grid_points(C.byref(g), points.ctypes.data, n), "terra_amd_probe_grid_points")
    return g, points


def probe_grid_over(lib, lo, hi, counts):
    """probe_grid cell-centred over the box lo .. hi, as terra_headless --bake-probes lays it: per axis spacing = (hi - lo) / count in binary32 (1 where the box
    has no extent), origin = lo + 0.5 * spacing"""
    f = np.float32
    spacing = [(f(h) - f(l)) / f(c) for l, h, c in zip(lo, hi, counts)]
    spacing = [s if s > 0 else f(1) for s in spacing]
    return probe_grid(lib, [f(l) + f(0.5) * s for l, s in zip(lo, spacing)], spacing, counts)


def probe_rays(lib, probes, cells: int, jitter=None):
    """terra_amd_probe_rays_device on the current torch stream: probes float32 [P, 8] in HBM (api.POINT_DTYPE records), jitter None (cell centres) or float32
    [cells * cells, 2] in HBM -> rays float32 [P, cells * cells, 8], the frame render_rays_device takes as it is (cell c of probe p at pixel (c, p))"""
    import torch
    n = _records(probes, 8, "probe_rays probes")
    if jitter is not None and not (isinstance(jitter, torch.Tensor) and jitter.is_cuda and jitter.dtype == torch.float32 and jitter.is_contiguous() and jitter.numel() == 2 * cells * cells):
        raise TerraAmdError("probe_rays takes jitter as a contiguous float32 tensor [cells * cells, 2] in HBM")
    rays = torch.empty((n, cells * cells, 8), dtype=torch.float32, device=probes.device)
    check(lib.probe_rays_device(probes.data_ptr(), n, cells, jitter.data_ptr() if jitter is not None else None, rays.data_ptr(), _current_stream()), "terra_amd_probe_rays_device")
    return rays


def sh_project(lib, results, rays, cells: int, batch: int = 0, sh=None):
    """terra_amd_sh_project_device on the current torch stream: results = the probe frame's running sums (a DeviceFramebuffer, or its results tensor), rays as
    probe_rays returns them -> sh float32 [P, 28] in HBM: api.PROBE_SH_DTYPE records (27 coefficients c[k][channel], then the bits of cells; probe_sh_host gives
    the records). batch > 0 averages into `sh`, the tensor an earlier call returned."""
    import torch
    results = results.results if isinstance(results, DeviceFramebuffer) else results
    n = _records(rays, 8, "sh_project rays")
    if _records(results, 4, "sh_project results") != n or n % (cells * cells):
        raise TerraAmdError("sh_project: one result and one ray per cell of every probe")
    probes = n // (cells * cells)
    if sh is None:
        if batch:
            raise TerraAmdError("sh_project: batch > 0 averages into the records of the earlier batches: pass sh")
        sh = torch.zeros((probes, 28), dtype=torch.float32, device=rays.device)
    elif _records(sh, 28, "sh_project sh") != probes:
        raise TerraAmdError("sh_project: one coefficient record per probe")
    check(lib.sh_project_device(results.data_ptr(), rays.data_ptr(), probes, cells, batch, sh.data_ptr(), _current_stream()), "terra_amd_sh_project_device")
    return sh


def probe_sh_host(sh) -> np.ndarray:
    """the coefficient records of a tensor [P, 28] as [P] api.PROBE_SH_DTYPE records on the host"""
    return sh.cpu().numpy().view(api.PROBE_SH_DTYPE).reshape(-1)


def sh_irradiance(lib, sh, points, grid: Optional[api.ProbeGrid] = None, index=None):
    """terra_amd_sh_irradiance_device on the current torch stream: sh [P, 28] as sh_project returns it, points float32 [n, 8] in HBM (api.POINT_DTYPE records: the
    normal is the lobe's axis, the position is looked at in grid mode), and either grid (trilinear blend of the grid's probes) or index (int32 [n] in HBM: one
    probe per query) -> float32 [n, 4]: (E_r, E_g, E_b, 0)"""
    import torch
    probes = _records(sh, 28, "sh_irradiance sh")
    n = _records(points, 8, "sh_irradiance points")
    if grid is None and not (isinstance(index, torch.Tensor) and index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and index.numel() == n):
        raise TerraAmdError("sh_irradiance without a grid takes index as a contiguous int32 tensor [n] in HBM")
    out = torch.empty((n, 4), dtype=torch.float32, device=points.device)
    check(lib.sh_irradiance_device(sh.data_ptr(), probes, C.byref(grid) if grid is not None else None, points.data_ptr(),
                                   index.data_ptr() if grid is None else None, n, out.data_ptr(), _current_stream()), "terra_amd_sh_irradiance_device")
    return out


def bake_probes(lib, scene, probes, cells: int = 16, batches: int = 1, jitter=None):
    """Order-2 SH of the radiance arriving at P probes (float32 [P, 8] in HBM: api.POINT_DTYPE records) -> sh float32 [P, 28] in HBM (probe_sh_host gives the [P]
    api.PROBE_SH_DTYPE records): probe_rays -> render_rays_device -> sh_project, all on the current torch stream. jitter None: the cell-centre rays, `batches`
    render calls of the scene's samples_per_pixel each into one frame, one projection. jitter = an int seed: every batch draws a fresh jitter array
    (torch.rand of [cells * cells, 2] from a device generator with that seed), renders a fresh frame along its rays and is averaged in by sh_project's batch."""
    import torch
    if batches < 1:
        raise TerraAmdError("bake_probes: batches must be at least 1")
    n = _records(probes, 8, "bake_probes probes")
    stream = _current_stream()
    fb = DeviceFramebuffer(cells * cells, n, device=probes.device)
    if jitter is None:
        rays = probe_rays(lib, probes, cells)
        for _ in range(batches):
            render_rays_device(lib, scene, rays, fb, stream=stream)
        return sh_project(lib, fb, rays, cells)
    gen = torch.Generator(device=probes.device)
    gen.manual_seed(int(jitter))
    sh = None
    for b in range(batches):
        if b:
            fb = DeviceFramebuffer(cells * cells, n, device=probes.device)
        rays = probe_rays(lib, probes, cells, torch.rand((cells * cells, 2), generator=gen, dtype=torch.float32, device=probes.device))
        render_rays_device(lib, scene, rays, fb, stream=stream)
        sh = sh_project(lib, fb, rays, cells, batch=b, sh=sh)
    return sh


# ---------------------------------------------------------------------------
# probe visibility (include/terra_amd.h "Probe visibility")
# ---------------------------------------------------------------------------

def probe_visibility_options(texels: int = 8, sharpness: int = 6, max_distance: float = 1.0, bias: float = 0.0, backface: bool = False) -> api.ProbeVisibility:
    """api.ProbeVisibility: maps of texels x texels (1 .. 16), the weight cos^(2^sharpness) (0 .. 8), max_distance for a miss and as the cap, and for the lookup the
    bias along the query's normal and the back-face term"""
    o = api.ProbeVisibility()
    o.texels, o.sharpness, o.max_distance, o.bias = int(texels), int(sharpness), float(max_distance), float(bias)
    o.flags = api.PROBE_VISIBILITY_BACKFACE if backface else 0
    return o


def probe_visibility(lib, hits, rays, cells: int, options: api.ProbeVisibility, map=None):
    """terra_amd_probe_visibility_device on the current torch stream: hits as intersect returns them for `rays` (float32 [P * K, 8] or [P, K, 8] in HBM), rays as
    probe_rays returns them -> map float32 [P, texels * texels, 4] in HBM: api.VISIBILITY_TEXEL_DTYPE records (the sums of w, w d, w d d, then the bits of cells;
    visibility_map_host gives the records). map = the tensor an earlier call returned: the sums are added to it."""
    import torch
    n = _records(rays, 8, "probe_visibility rays")
    if _records(hits, 8, "probe_visibility hits") != n or n % (cells * cells):
        raise TerraAmdError("probe_visibility: one hit and one ray per cell of every probe")
    probes, mm = n // (cells * cells), options.texels * options.texels
    accumulate = map is not None
    if map is None:
        map = torch.zeros((probes, mm, 4), dtype=torch.float32, device=rays.device)
    elif _records(map, 4, "probe_visibility map") != probes * mm:
        raise TerraAmdError("probe_visibility: texels * texels records per probe")
    check(lib.probe_visibility_device(hits.data_ptr(), rays.data_ptr(), probes, cells, C.byref(options), int(accumulate), map.data_ptr(), _current_stream()), "terra_amd_probe_visibility_device")
    return map


def visibility_map_host(vis_map) -> np.ndarray:
    """the texels of a tensor [P, m * m, 4] as [P, m * m] api.VISIBILITY_TEXEL_DTYPE records on the host"""
    return vis_map.cpu().numpy().view(api.VISIBILITY_TEXEL_DTYPE).reshape(vis_map.shape[0], -1)


def sh_irradiance_visible(lib, sh, vis_map, points, grid: api.ProbeGrid, options: api.ProbeVisibility):
    """terra_amd_sh_irradiance_visible_device on the current torch stream: sh [P, 28] as sh_project returns it, vis_map [P, texels * texels, 4] as probe_visibility
    returns it, points float32 [n, 8] in HBM (api.POINT_DTYPE records), the grid of the P probes -> float32 [n, 4]: (E_r, E_g, E_b, 0), every probe weighted by its
    visibility from the query"""
    import torch
    probes = _records(sh, 28, "sh_irradiance_visible sh")
    n = _records(points, 8, "sh_irradiance_visible points")
    if _records(vis_map, 4, "sh_irradiance_visible map") != probes * options.texels * options.texels:
        raise TerraAmdError("sh_irradiance_visible: texels * texels map records per probe")
    if grid is None:
        raise TerraAmdError("sh_irradiance_visible is a grid lookup: pass the grid")
    out = torch.empty((n, 4), dtype=torch.float32, device=points.device)
    check(lib.sh_irradiance_visible_device(sh.data_ptr(), vis_map.data_ptr(), probes, C.byref(grid), C.byref(options), points.data_ptr(), n, out.data_ptr(), _current_stream()),
          "terra_amd_sh_irradiance_visible_device")
    return out


def bake_probe_visibility(lib, scene, probes, cells: int, options: api.ProbeVisibility, batches: int = 1, jitter=None):
    """The visibility maps of P probes (float32 [P, 8] in HBM: api.POINT_DTYPE records) -> map float32 [P, texels * texels, 4] in HBM: probe_rays -> intersect ->
    probe_visibility, all on the current torch stream. jitter None: the cell-centre rays, once (the distances are exact: further batches would add the same sums
    again, so `batches` must be 1). jitter = an int seed: every batch draws a fresh jitter array the way bake_probes does (torch.rand of [cells * cells, 2] from a
    device generator with that seed) and adds its sums to the map."""
    import torch
    if batches < 1:
        raise TerraAmdError("bake_probe_visibility: batches must be at least 1")
    n = _records(probes, 8, "bake_probe_visibility probes")
    if jitter is None:
        if batches != 1:
            raise TerraAmdError("bake_probe_visibility: batches > 1 needs a jitter seed (the cell-centre rays give the same distances every time)")
        rays = probe_rays(lib, probes, cells)
        return probe_visibility(lib, intersect(lib, scene, rays.view(-1, 8)), rays, cells, options)
    gen = torch.Generator(device=probes.device)
    gen.manual_seed(int(jitter))
    vis_map = None
    for _ in range(batches):
        rays = probe_rays(lib, probes, cells, torch.rand((cells * cells, 2), generator=gen, dtype=torch.float32, device=probes.device))
        vis_map = probe_visibility(lib, intersect(lib, scene, rays.view(-1, 8)), rays, cells, options, map=vis_map)
    return vis_map


def render_device_sharded(lib, cam, scene, fb: DeviceFramebuffer, tile: int, rank: int, world: int, stream=None):
    check(lib.render_device_sharded(C.byref(cam), scene, fb.pixels.data_ptr(), fb.results.data_ptr(), fb.width, fb.height,
                                    0, 0, fb.width, fb.height, tile, rank, world, None, stream), "terra_amd_render_device_sharded")


# ---------------------------------------------------------------------------
# tile sharding across ranks (one process per GPU) and the single gather
# ---------------------------------------------------------------------------

def shard_tiles(width: int, height: int, tile: int, rank: int, world: int):
    """tile ids (row-major in the frame) owned by `rank`: t % world == rank (same rule as the kernel)"""
    tx, ty = -(-width // tile), -(-height // tile)
    return [t for t in range(tx * ty) if t % world == rank]


def packed_floats_per_rank(width: int, height: int, tile: int, world: int) -> int:
    """floats in one rank's packed gather buffer (padded to rank 0's tile count): 7 floats = 28 B per pixel"""
    tx, ty = -(-width // tile), -(-height // tile)
    most = -(-(tx * ty) // world)
    return most * tile * tile * 7


def gather_frame(fb_pack, fb_unpack, width, height, tile, rank, world, dist, make_buffer, dst=0, mark=None):
    """One gather of every rank's packed tiles to `dst`, then unpack there.

    fb_pack(rank) -> 1-D float32 tensor holding this rank's tiles in the packed layout
    fb_unpack(src_rank, packed) writes rank src_rank's tiles into the destination frame (called on dst only)
    dist: torch.distributed (backend nccl == RCCL on the GPU box, gloo in CPU tests)
    mark(name): optional, called after each phase is QUEUED ("packed", "gathered", "unpacked") -- bench.py records stream events there
    """
    mark = mark or (lambda name: None)
    mine = fb_pack(rank)
    mark("packed")
    if world == 1 and not (dist is not None and dist.is_available() and dist.is_initialized()):
        mark("gathered"); mark("unpacked")
        return
    # (one rank WITH a process group -- bench.py's TERRA_BENCH_DIST1 self-test -- still issues the collective: the gather of a group of one)
    n = packed_floats_per_rank(width, height, tile, world)
    assert mine.numel() == n
    if rank == dst:
        bufs = [make_buffer(n) for _ in range(world)]
        dist.gather(mine, gather_list=bufs, dst=dst)
        mark("gathered")
        for src in range(world):
            if src != dst:
                fb_unpack(src, bufs[src])
    else:
        dist.gather(mine, gather_list=None, dst=dst)
        mark("gathered")
    mark("unpacked")
