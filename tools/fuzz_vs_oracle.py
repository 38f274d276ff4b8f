"""Randomised device-vs-oracle run on the GPU (not a unit test): random triangle soups (2..2500 triangles, so all three
kernel layouts: LDS-resident, global/decoupled, fast tree), random preset mixes incl. Phong / GGX / glass, all seven
integrators, random sample splits. The device image in replica mode (tree mode 0) must equal the oracle's (device-twin math)
bit for bit (NaNs: same positions), and the fast tree (mode 1) and the automatic mode (2: leaf-box cull / fast tree when the
numeric containment check passes) must equal the replica mode. FUZZ_SCALE multiplies every coordinate: 1 and 2 stay inside the
check's range (+-13), 4 puts the camera outside (per-call fallback), 100 everything (commit-time fallback).
    python tools/fuzz_vs_oracle.py [iterations] [seed]"""
import torch  # first
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from terra_amd import api, runtime, scenes

n_iter = int(sys.argv[1]) if len(sys.argv) > 1 else 40
SCALE = float(os.environ.get("FUZZ_SCALE", "1"))       # multiplies every coordinate (scene and camera): the 1e-4 box margins do not scale with it
EXT = os.environ.get("FUZZ_EXT", "0") == "1"
rs = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
rs_pairs = np.random.RandomState((int(sys.argv[2]) if len(sys.argv) > 2 else 1) ^ 0x9A125)      # terra_amd_set_leaf_pairs, drawn apart from the cases
lib = runtime.load()
orc = api.TerraLib(os.path.join(ROOT, "oracle", "liboracle.so"), "orc_")
orc.fn("orc_set_math_mode", None, [C.c_int])(1)
orp = orc.fn("orc_render_pixels", None, [C.POINTER(api.TerraCamera), C.c_void_p, C.POINTER(api.TerraFramebuffer)] + [C.c_size_t] * 4 + [C.c_uint64, C.c_void_p])


def random_texture(scale=1.0):
    """FUZZ_EXT=1: random size, filter, address mode, depth and 1-4 components"""
    th, tw, c = int(rs.randint(1, 9)), int(rs.randint(1, 12)), int(rs.randint(1, 5))
    data = (rs.uniform(0, scale, size=(th, tw, c)).astype(np.float32) if rs.randint(2) else rs.randint(0, 256, size=(th, tw, c)).astype(np.uint8))
    return scenes.TextureDesc(data, filter=int(rs.randint(0, 2)), address_mode=int(rs.randint(0, 3)))


def soup(n_tris, n_objects):
    objs = []
    per = max(1, n_tris // n_objects); left = n_tris
    for k in range(n_objects):
        n = per if k < n_objects - 1 else left
        if n <= 0: break
        left -= n
        c = rs.uniform(-2, 2, size=(n, 1, 3)); tris = ((c + rs.uniform(-0.5, 0.5, size=(n, 3, 3))) * SCALE).astype(np.float32)
        e1 = tris[:, 1] - tris[:, 0]; e2 = tris[:, 2] - tris[:, 0]
        nrm = np.cross(e1, e2); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-20)
        nrm = np.repeat(nrm[:, None, :], 3, axis=1).astype(np.float32)
        kind = str(rs.choice(["diffuse", "diffuse", "phong", "ggx", "glass"]))
        m = scenes.Material(kind=kind, albedo=tuple(rs.uniform(0.2, 0.9, 3)), emissive=(4.0, 3.0, 2.0) if k == 0 else (0.0, 0.0, 0.0),
                            specular_color=tuple(rs.uniform(0.1, 0.9, 3)), specular_intensity=float(rs.choice([1.0, 8.0, 30.5])), roughness=float(rs.uniform(0.05, 0.9)), ior=1.5)
        uv = rs.uniform(0, 1, size=(n, 3, 2)).astype(np.float32)
        if EXT and rs.randint(3) == 0:      # FUZZ_EXT=1: some materials with a textured albedo / emissive, texcoords (texel units) across several tiles and below 0
            if kind in ("diffuse", "phong"): m.albedo_texture = random_texture()
            if k == 0 and rs.randint(2): m.emissive_texture = random_texture(6.0)
            uv = rs.uniform(-3, 30, size=(n, 3, 2)).astype(np.float32)
        objs.append(scenes.ObjectDesc(tris, nrm, uv, m))
    return objs


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


decided = {"fast": 0, "cull": 0, "replica": 0}
faults_fn = lib.fn("terra_amd_debug_faults", C.c_longlong, [C.c_void_p]); faults = 0
bad = 0
for it in range(n_iter):
    n = int(rs.choice([2, 9, 40, 150, 400, 1200, 2500])); W, H = int(rs.randint(20, 70)), int(rs.randint(16, 50))
    integ = int(rs.randint(0, 7)); split = int(rs.choice([1, 1, 2, 4])); spp = split * int(rs.randint(1, 3))
    d = scenes.SceneDesc(objects=soup(n, int(rs.randint(1, 5))), width=W, height=H, spp=spp, bounces=int(rs.randint(0, 6)), integrator=integ,
                         camera_position=(0.0, 0.0, -6.0 * SCALE), tonemap=int(rs.randint(0, 5)), environment=(0.2, 0.3, 0.4), environment_lighting=bool(rs.randint(2)),
                         jitter=float(rs.choice([0.0, 0.5])))      # jitter 0 on odd frame sizes gives rays with exactly zero direction components (the exact slab path)
    if EXT:     # FUZZ_EXT=1: the unpinned extensions too (and textured materials, soup()) -- a lat-long environment texture, environment importance sampling, the pixel sampler feeding bounce 0
        if rs.randint(2):
            th, tw = int(rs.randint(1, 12)), int(rs.randint(1, 20))
            tex = rs.uniform(0, 3, size=(th, tw, 3)).astype(np.float32) if rs.randint(2) else rs.randint(0, 256, size=(th, tw, 3)).astype(np.uint8)
            if rs.randint(3) == 0: tex[rs.randint(th), rs.randint(tw)] = tex.max() * (40 if tex.dtype == np.float32 else 1)
            d.environment_texture = scenes.TextureDesc(tex, address_mode=int(rs.randint(0, 3))); d.environment_lighting = True
            d.environment_sampling = bool(rs.randint(2))
        m = int(rs.randint(3))
        if m == 1: d.sampling = api.kTerraSamplingMethodHalton; d.sampler_integration = True
        if m == 2 and split == 1: d.sampling = api.kTerraSamplingMethodStratified; d.strata = int(rs.randint(1, 4)); d.sampler_integration = bool(rs.randint(2))
    cam = scenes.camera_of(d)
    so = scenes.build_scene(orc, d); fo = api.Framebuffer(orc, W, H)
    dchunk = scenes.SceneDesc(**{**d.__dict__, "spp": spp // split}); sc = scenes.build_scene(orc, dchunk)
    for _ in range(split):
        orp(C.byref(cam), sc, C.byref(fo.fb), 0, 0, W, H, scenes.FRAME_SEED, None)
    outs = []
    for tree in (0, 1, 2):
        lib.clear_error()
        # (work counters on or off at random: the counting kernels are separate instantiations, and only the ones WITHOUT counters take the light-sample rays' shortcut)
        s = scenes.build_scene(lib, d, tree_mode=tree, counters=bool(rs.randint(2))); runtime.check(lib.set_sample_split(s, split))
        if hasattr(lib, "set_leaf_pairs"):      # the pair form of ranked launches (scenes of quads): off or on (the default), from a stream of its own, so that a seed's cases stay the ones earlier logs name
            runtime.check(lib.set_leaf_pairs(s, int(rs_pairs.randint(2))))
        if hasattr(lib, "set_job_order"):      # the order LDS-resident launches hand their pixel blocks out in: off, the default (off at these frame sizes), or on for launches of any size
            runtime.check(lib.set_job_order(s, int(rs.choice([0, 1, 2, 2]))))
        if tree and hasattr(lib, "debug_fast_stack_lds"):      # the fast tree's stack: sometimes only 1-3 entries in LDS, so that the HBM part is exercised (the image must not change)
            runtime.check(lib.debug_fast_stack_lds(s, int(rs.choice([0, 0, 1, 2, 3]))))
        fb = runtime.DeviceFramebuffer(W, H)
        runtime.check(lib.render_device(C.byref(cam), s, fb.pixels.data_ptr(), fb.results.data_ptr(), W, H, 0, 0, W, H, None, None))
        torch.cuda.synchronize()
        outs.append((fb.results_host()["acc"].copy(), fb.pixels_host().copy()))
        faults += max(0, faults_fn(s))
        if tree == 2:
            ti = runtime.TraversalInfo(); runtime.check(lib.traversal_info(s, C.byref(ti)))
            decided["fast" if ti.fast_tree else "cull" if ti.leaf_cull else "replica"] += 1
        lib.scene_destroy(s)
    ok0 = bits_equal(outs[0][0], fo.results["acc"]) and bits_equal(outs[0][1], fo.pixels)
    ok1 = bits_equal(outs[1][0], outs[0][0]) and bits_equal(outs[1][1], outs[0][1])
    ok2 = bits_equal(outs[2][0], outs[0][0]) and bits_equal(outs[2][1], outs[0][1])
    if not (ok0 and ok1 and ok2):
        bad += 1; print("MISMATCH", dict(it=it, tris=n, W=W, H=H, integ=integ, split=split, spp=spp, bounces=d.bounces, tonemap=d.tonemap, env=d.environment_lighting, vs_oracle=ok0, fast_vs_ref=ok1, auto_vs_ref=ok2,
                                         kinds=[o.material.kind for o in d.objects], env_tex=d.environment_texture is not None, env_sampling=d.environment_sampling, sampling=d.sampling, sampler=d.sampler_integration))
    fo.destroy(); orc.scene_destroy(so); orc.scene_destroy(sc)
    if (it + 1) % 1000 == 0: print(f"  {it + 1} cases, {bad} mismatches so far", file=sys.stderr, flush=True)      # (a long silent run on the GPU box is taken for a hang)
print(f"{n_iter} cases at scale {SCALE:g}{' with the extensions' if EXT else ''}, {bad} mismatches, {faults} bounds faults, automatic mode chose {decided}, last error: '{runtime.last_error()}'")
sys.exit(1 if bad or faults else 0)
