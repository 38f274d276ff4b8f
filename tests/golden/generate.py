"""Generates the golden vectors in this directory from the COMPILED REFERENCE
(oracle/_ref/libterra_ref.so, built by `make -C oracle ref` from the unmodified
sources under /root/reference with entropy pinned -- see oracle/ref_wrapper.c).

Run in the build container only:   python tests/golden/generate.py

What is stored is data: inputs and the reference's outputs (SURVEY.md section 4's
pin list). No reference source travels. The reference has no tests, golden
images or known-answer vectors of its own, so these are the
pins of the oracle: tests/test_oracle_golden.py replays them bit-for-bit.
"""
from __future__ import annotations

import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))
import harness as H  # noqa: E402
from terra_amd import api, scenes  # noqa: E402


def save(name, **arrays):
    np.savez_compressed(HERE / f"{name}.npz", **arrays)
    return {k: {"shape": list(np.shape(v)), "dtype": str(np.asarray(v).dtype), "sha256": H.digest(np.asarray(v))} for k, v in arrays.items()}


def main():
    assert H.have_reference(), "needs /root/reference"
    H.build_reference()
    ref = H.Unit("ref")
    manifest = {"generator": "tests/golden/generate.py", "source": "compiled reference (oracle/_ref), gcc -O2 -ffp-contract=off, glibc 2.35",
                "frame_seed": hex(scenes.FRAME_SEED), "files": {}}

    # A2: camera-jitter PCG32
    seeds = np.array([0, 1, 0x5EED0001, 0xFFFFFFFF], np.uint32)
    manifest["files"]["pcg"] = save("pcg", seeds=seeds, floats=ref.pcg(seeds, 64))

    # A11: camera
    r = H.rng(21)
    d = scenes.cornell_box(1920, 1080)
    cam = scenes.camera_of(d)
    xy = np.stack([r.randint(0, 1920, 256), r.randint(0, 1080, 256)], axis=1).astype(np.uint32)
    xy[:4] = [[0, 0], [1919, 0], [0, 1079], [1919, 1079]]
    rr = r.uniform(0, 1, size=(256, 2)).astype(np.float32)
    rr[:2] = [[0, 0], [1, 1]]
    manifest["files"]["camera"] = save("camera", xy=xy, r=rr, jitter=np.float32(0.5), dirs=ref.camera_dirs(cam, 1920, 1080, xy, 0.5, rr))
    cam2 = api.TerraCamera(); cam2.position = api.f3((0.3, 1.2, -2.0)); cam2.direction = api.f3((0.2, -0.1, 1.0)); cam2.up = api.f3((0.05, 1.0, 0.0)); cam2.fov = 60.0
    manifest["files"]["camera_tilted"] = save("camera_tilted", xy=xy, r=rr, jitter=np.float32(0.25), dirs=ref.camera_dirs(cam2, 1920, 1080, xy, 0.25, rr))

    # A6: slab test
    o, dd, boxes = H.aabb_cases()
    hit, tmin, tmax = ref.ray_aabb(o, dd, boxes)
    manifest["files"]["ray_aabb"] = save("ray_aabb", o=o, d=dd, boxes=boxes, hit=hit, tmin=tmin, tmax=tmax)

    # A7 / A7': triangle tests
    o, dd, tris = H.watertight_cases()
    hit, out = ref.watertight(o, dd, tris)
    manifest["files"]["watertight"] = save("watertight", o=o, d=dd, tris=tris, hit=hit, out=out)
    hit, out = ref.moller_trumbore(o, dd, tris)
    manifest["files"]["moller_trumbore"] = save("moller_trumbore", o=o, d=dd, tris=tris, hit=hit, out=out)

    # A16 + A5 + A4/A8 on Cornell-32
    L = ref.L
    dsc = scenes.cornell_box(256, 256, 4)
    scene = scenes.build_scene(L, dsc)
    manifest["files"]["bvh_cornell"] = save("bvh_cornell", nodes=ref.bvh_nodes(scene))
    o, dd = H.scene_rays(31, 4096)
    found, prim, point = ref.bvh_traverse(scene, o, dd)
    manifest["files"]["bvh_traverse"] = save("bvh_traverse", o=o, d=dd, found=found, prim=prim, point=point)
    o, dd = H.scene_rays(32, 2048)
    obj, tri, point, surf = ref.raycast(scene, o, dd)
    manifest["files"]["raycast"] = save("raycast", o=o, d=dd, obj=obj, tri=tri, point=point, surface=surf)
    L.scene_destroy(scene)

    # A12/A13: BSDF presets
    for kind_id, name in [(0, "diffuse"), (1, "phong")]:
        surf, e, wo = H.bsdf_cases(41 + kind_id, 2048, kind_id)
        wi, pdf, f, surf_after = ref.bsdf(kind_id, surf, e, wo)
        manifest["files"][f"bsdf_{name}"] = save(f"bsdf_{name}", surfaces=surf, e=e, wo=wo, wi=wi, pdf=pdf, f=f, pick=surf_after[:, 32])

    # A3/A9: terra_trace per primary ray, every integrator, diffuse and Phong scenes
    for sname, mk in [("cornell", scenes.cornell_box), ("phong", scenes.cornell_phong)]:
        for integ in range(7):
            dsc = mk(64, 64, 1, integrator=integ)
            scene = scenes.build_scene(L, dsc)
            o, dd = H.scene_rays(50 + integ, 1024)
            stateB, incB = H.stream_states(60 + integ, 1024)
            rad, calls = ref.trace(scene, o, dd, stateB, incB)
            manifest["files"][f"trace_{sname}_{integ}"] = save(f"trace_{sname}_{integ}", o=o, d=dd, stateB=stateB, incB=incB, radiance=rad, rand_calls=calls.astype(np.uint16))
            L.scene_destroy(scene)

    # A1: end-to-end. Config 1 (BASELINE.json configs[0]): Cornell, 256x256, 4 spp, Simple, fixed seed
    out = ref.render_pixels(scenes.cornell_box(256, 256, 4))
    manifest["files"]["render_config1"] = save("render_config1", acc=out["acc"], samples=np.int32(out["samples"][0, 0]), rand_calls=out["rand_calls"].astype(np.uint8))
    manifest["config1"] = {"pixels_sha256": H.digest(out["pixels"]), "pixels_fnv1a64": hex(H.fnv1a(out["pixels"])), "mean": float(out["pixels"].mean())}
    # small crops: other integrators / tonemaps / Phong / two accumulating passes
    small = {}
    for sname, mk in [("cornell", scenes.cornell_box), ("phong", scenes.cornell_phong)]:
        for integ in range(7):
            for tm in ([0, 1, 2, 3, 4] if (integ == 0 and sname == "cornell") else [0]):
                o2 = ref.render_pixels(mk(48, 32, 3, integrator=integ, tonemap=tm), passes=2)
                key = f"{sname}_i{integ}_t{tm}"
                small[key + "_pixels"] = o2["pixels"]; small[key + "_acc"] = o2["acc"]; small[key + "_calls"] = o2["rand_calls"].astype(np.uint16)
    # stratified sampling rounds spp up (reference src/Terra.c:519-527)
    o3 = ref.render_pixels(scenes.cornell_box(16, 16, 5, sampling=api.kTerraSamplingMethodStratified, strata=2))
    small["stratified_pixels"] = o3["pixels"]; small["stratified_samples"] = o3["samples"]
    # a tile of a larger frame (tile offsets, non-square aspect)
    o4 = ref.render_pixels(scenes.cornell_box(160, 90, 2), rect=(48, 16, 64, 32))
    small["tile_pixels"] = o4["pixels"]; small["tile_samples"] = o4["samples"]
    manifest["files"]["render_small"] = save("render_small", **small)

    # config 3 geometry: the ~100k-triangle hall (deep reference-tree traversal), small frames
    hall = {}
    for integ, (w, h, spp) in {0: (160, 90, 2), 1: (64, 36, 1)}.items():
        o5 = ref.render_pixels(scenes.sponza_hall(w, h, spp, integrator=integ))
        hall[f"i{integ}_pixels"] = o5["pixels"]; hall[f"i{integ}_calls"] = o5["rand_calls"].astype(np.uint16)
    dh = scenes.sponza_hall(64, 36, 1)
    sc = scenes.build_scene(L, dh)
    nodes = ref.bvh_nodes(sc)
    hall["bvh_sha256"] = np.frombuffer(bytes.fromhex(H.digest(nodes)), dtype=np.uint8)
    hall["bvh_nodes"] = np.int64(len(nodes))
    o, dd = H.scene_rays(71, 512, box=((-9.5, 0.3, -4.5), (9.5, 7.5, 4.5)))
    found, prim, point = ref.bvh_traverse(sc, o, dd)
    hall["trav_found"] = found; hall["trav_prim"] = prim; hall["trav_point"] = point
    L.scene_destroy(sc)
    manifest["files"]["render_hall"] = save("render_hall", **hall)

    # the same hall with every coordinate (scene and camera) x 100: outside the +-13-unit range in which the 1e-4 box margins provably exceed rounding error;
    # the product's automatic mode renders it with the fast tree and the reference's reachability replayed -- this is what it has to reproduce
    from tools.scaled_hall import scaled
    hall100 = {}
    for integ, (w, h, spp) in {0: (160, 90, 2), 1: (64, 36, 1)}.items():
        o5 = ref.render_pixels(scaled(scenes.sponza_hall(w, h, spp, integrator=integ), 100.0))
        hall100[f"i{integ}_pixels"] = o5["pixels"]; hall100[f"i{integ}_calls"] = o5["rand_calls"].astype(np.uint16)
    manifest["files"]["render_hall_x100"] = save("render_hall_x100", **hall100)

    # textured attributes (byte/float textures, point/bilinear, wrap/clamp, textured emissive)
    tex = {}
    for integ in (0, 1, 2):
        o6 = ref.render_pixels(scenes.cornell_textured(64, 48, 3, integrator=integ), passes=2)
        tex[f"i{integ}_pixels"] = o6["pixels"]; tex[f"i{integ}_calls"] = o6["rand_calls"].astype(np.uint16)
    manifest["files"]["render_textured"] = save("render_textured", **tex)

    # SURVEY 8f N4 (unit level): stratified / Halton samplers, 1D / 2D distributions (reference src/Terra.c:703-846)
    smp = {}
    seeds = np.array([0, 7, 0x5EED0001, 0xFFFFFFFF], np.uint32)
    for strata, samples in ((1, 1), (2, 3), (4, 16), (7, 2)):
        smp[f"strat_{strata}_{samples}"] = ref.stratified(seeds, strata, samples, strata * strata * samples)
    smp["seeds"] = seeds
    smp["halton_0"] = ref.halton(0, 4096)
    smp["halton_far"] = ref.halton(2 ** 30, 512)
    tables, e, t2, e12 = H.sampler_cases()
    smp["e"] = e; smp["e12"] = e12
    for name, f in tables.items():
        o7 = ref.distribution_1d(f, e)
        smp[f"d1_{name}_f"] = f
        for k, v in o7.items():
            smp[f"d1_{name}_{k}"] = v
    for name, f in t2.items():
        o8 = ref.distribution_2d(f, e12)
        smp[f"d2_{name}_f"] = f
        for k, v in o8.items():
            smp[f"d2_{name}_{k}"] = v
    manifest["files"]["samplers"] = save("samplers", **smp)

    # the texture lookups texel by texel, with the mask of where the reference defines them
    manifest["files"]["texture_sample"] = save("texture_sample", **texture_block(ref))
    manifest["files"]["render_atlas"] = save("render_atlas", **atlas_block(ref))

    (HERE / "manifest.json").write_text(json.dumps(manifest, indent=1))
    total = sum(p.stat().st_size for p in HERE.glob("*.npz"))
    print(f"wrote {len(manifest['files'])} fixtures, {total / 1e6:.2f} MB")


# ---------------------------------------------------------------------------------------------------------------------------------
# texture lookups, texel by texel (terra_texture_sample / terra_texture_sample_latlong, src/Terra.c:368-477)
# ---------------------------------------------------------------------------------------------------------------------------------
TEX_SIZES = [(1, 1), (1, 13), (13, 1), (5, 3), (13, 3), (16, 16), (65535, 1), (1, 65535)]      # (W, Ht): 5x3 / 13x3 byte rows are no multiple of four
TEX_SAMPLES = 128


def texture_texels(W, Ht, depth, seed):
    """W*Ht*3 elements, of which a case of c components uses the first W*Ht*c. The two long textures tile a random run of prime length, so that the file
    stays small when compressed while neighbouring texels still differ"""
    r = H.rng(seed)
    n = W * Ht * 3
    m = min(n, 4093)
    base = r.randint(0, 256, m).astype(np.uint8) if depth == 1 else r.uniform(0, 4, m).astype(np.float32)
    return np.resize(base, n)


def texture_defined(W, Ht, comps, filt, addr, uv):
    """From the integer addressing alone: True where the reference's result is defined. Exactly three things clear it: components < 3 and a read that
    touches the last texel in memory (2 components) or one of the last two (1); mirror mode, a read in an odd tile with x % W == 0 or y % Ht == 0 (the
    reference addresses column W / row Ht there); uv outside (-1, 2^32) or not finite."""
    uv = np.asarray(uv, np.float32)
    ok = np.isfinite(uv).all(axis=1) & (uv > -1).all(axis=1) & (uv < 2.0 ** 32).all(axis=1)
    t = np.where(ok[:, None], uv, 0).astype(np.float64)
    ix = np.trunc(t[:, 0]).astype(np.int64); iy = np.trunc(t[:, 1]).astype(np.int64)
    reads = [(ix, iy)]
    if filt == 1:
        x2 = np.minimum(ix + 1, W - 1); y2 = np.minimum(iy + 1, Ht - 1)
        reads = [(ix, iy), (x2, iy), (ix, y2), (x2, y2)]
    for x, y in reads:
        if addr == 2:
            xa, ya = np.minimum(x, W - 1), np.minimum(y, Ht - 1)
        elif addr == 0:
            xa, ya = x % W, y % Ht
        else:
            odd = (x // W) % 2 == 1
            ok &= ~(odd & ((x % W == 0) | (y % Ht == 0)))
            xa = np.where(odd, np.minimum(W - x % W, W - 1), x % W); ya = np.where(odd, np.minimum(Ht - y % Ht, Ht - 1), y % Ht)
        if comps < 3:
            ok &= (ya * W + xa) < W * Ht - (3 - comps)
    return ok


def texture_uv(W, Ht, comps, filt, addr, seed):
    """TEX_SAMPLES coordinates in texel units: uniform over several tiles, exact integers, the last texel, W - 0.5, W, 2W, values in (-1, 0), around 2^24
    and up to just below 2^32 -- drawn from a larger pool so that at most a fifth of them lie where the reference is undefined (a 1- or 2-component
    texture read with the bilinear filter is defined in the first tile only, a mirrored 1xN one in even tiles only)"""
    r = H.rng(seed)
    f32 = np.float32
    special = []
    for a, b in ((W, Ht), (Ht, W)):
        vals = [0.0, 1.0, a - 1.0, a - 0.5, float(a), 2.0 * a, a - 1 + 0.999, -0.25, -0.999, -1e-30, 2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 31, float(np.nextafter(f32(2.0 ** 32), f32(0)))]
        special.append(np.array(vals, np.float32))
    sx, sy = special
    k = len(sx)
    spec = np.stack([sx, r.uniform(0, 3 * Ht, k).astype(np.float32)], axis=1)
    spec = np.concatenate([spec, np.stack([r.uniform(0, 3 * W, k).astype(np.float32), sy], axis=1), np.stack([sx, sy], axis=1)])
    pool = np.stack([r.uniform(0, 3 * W, 6000), r.uniform(0, 3 * Ht, 6000)], axis=1).astype(np.float32)
    pool[:2000] = np.stack([r.uniform(0, W, 2000), r.uniform(0, Ht, 2000)], axis=1).astype(np.float32)          # the first tile
    pool[2000:2600] = np.floor(pool[2000:2600])                                                               # exact integers
    pool[2600:2700, 0] = r.uniform(-1, 0, 100); pool[2700:2800, 1] = r.uniform(-1, 0, 100)
    d_spec = texture_defined(W, Ht, comps, filt, addr, spec); d_pool = texture_defined(W, Ht, comps, filt, addr, pool)
    budget = TEX_SAMPLES // 5
    keep = np.concatenate([spec[d_spec], spec[~d_spec][:budget // 2], pool[~d_pool][:budget - budget // 2]])[:TEX_SAMPLES]
    fill = pool[d_pool]
    assert len(keep) + len(fill) >= TEX_SAMPLES, (W, Ht, comps, filt, addr, len(keep), len(fill))
    uv = np.concatenate([keep, fill[r.permutation(len(fill))[:TEX_SAMPLES - len(keep)]]])
    return np.ascontiguousarray(uv[r.permutation(len(uv))], np.float32)


def texture_cases():
    """(W, Ht, components, depth, filter, address): every filter x address x depth x components combination, each on two or three of TEX_SIZES (1x1 only
    with three components: with fewer, every read touches the last texel), then trilinear and anisotropic once each (the reference returns zero)"""
    cases = []
    for filt in (0, 1):
        for addr in (0, 1, 2):
            for depth in (1, 4):
                for si, (W, Ht) in enumerate(TEX_SIZES):
                    comps = 3 if si == 0 else 1 + (si + filt + addr + depth) % 3
                    cases.append((W, Ht, comps, depth, filt, addr))
    cases += [(5, 3, 3, 1, 2, 0), (5, 3, 3, 4, 3, 2)]
    return cases


def texture_block(ref):
    g = {}
    for si, (W, Ht) in enumerate(TEX_SIZES):
        for depth in (1, 4):
            g[f"texels_{W}x{Ht}_d{depth}"] = texture_texels(W, Ht, depth, 700 + 2 * si + depth)
    cases = texture_cases()
    g["cases"] = np.array(cases, np.int32)
    seen = set()
    g["uv"] = np.zeros((len(cases), TEX_SAMPLES, 2), np.float32); g["out"] = np.zeros((len(cases), TEX_SAMPLES, 3), np.float32)
    g["defined"] = np.zeros((len(cases), TEX_SAMPLES), bool)
    for k, (W, Ht, comps, depth, filt, addr) in enumerate(cases):
        data = g[f"texels_{W}x{Ht}_d{depth}"][:W * Ht * comps].reshape(Ht, W, comps).copy()      # (its own allocation, as terra_texture_init makes one)
        uv = texture_uv(W, Ht, comps, filt, addr, 800 + k)
        defined = texture_defined(W, Ht, comps, filt, addr, uv)
        out = np.zeros((len(uv), 3), np.float32)
        out[defined] = ref.texture_sample(data, filt, addr, uv[defined])      # (elsewhere the reference reads outside its allocation: it is not asked)
        # the three conditions on the mask
        if comps == 3 and addr != 1:
            assert defined.all(), (k, cases[k])
        assert (~defined).sum() <= 0.3 * len(uv) and defined.sum() >= 100, (k, cases[k], int(defined.sum()))
        if filt > 1:
            assert not out.any()
        g["uv"][k] = uv; g["out"][k] = out; g["defined"][k] = defined
        seen.add((filt, addr, depth, comps))
    assert all((f, a, d, c) in seen for f in (0, 1) for a in (0, 1, 2) for d in (1, 4) for c in (1, 2, 3))
    # the lat-long lookup (nearest texel by direction): three components, every address mode
    r = H.rng(790)
    dirs = r.normal(size=(256, 3)).astype(np.float32)
    dirs[:64] *= r.uniform(0.01, 100, size=(64, 1)).astype(np.float32)          # not normalised
    g["ll_dirs"] = dirs
    ll = [(16, 8, 1, 0), (7, 5, 4, 2), (13, 3, 1, 1), (16, 16, 4, 0)]
    g["ll_cases"] = np.array(ll, np.int32)
    for k, (W, Ht, depth, addr) in enumerate(ll):
        size = TEX_SIZES.index((W, Ht)) if (W, Ht) in TEX_SIZES else None
        data = (g[f"texels_{W}x{Ht}_d{depth}"] if size is not None else texture_texels(W, Ht, depth, 780 + k))[:W * Ht * 3].reshape(Ht, W, 3).copy()
        g[f"ll_texels_{k}"] = data
        g[f"ll_out_{k}"] = ref.texture_latlong(data, addr, dirs)
    return g


def atlas_block(ref):
    """the atlas wall restricted to what the reference defines (scenes.atlas(reference_defined=True)): integrators 0-2, two accumulating passes"""
    g = {}
    for integ in (0, 1, 2):
        o = ref.render_pixels(scenes.atlas(64, 48, 3, integrator=integ, reference_defined=True), passes=2)
        g[f"i{integ}_pixels"] = o["pixels"]; g[f"i{integ}_calls"] = o["rand_calls"].astype(np.uint16)
    return g


def texture_only():
    """python tests/golden/generate.py texture_sample: the texture blocks (texture_sample, render_atlas) alone, into the manifest as it stands"""
    assert H.have_reference(), "needs /root/reference"
    H.build_reference()
    manifest = json.loads((HERE / "manifest.json").read_text())
    manifest["files"]["texture_sample"] = save("texture_sample", **texture_block(H.Unit("ref")))
    manifest["files"]["render_atlas"] = save("render_atlas", **atlas_block(H.Unit("ref")))
    (HERE / "manifest.json").write_text(json.dumps(manifest, indent=1))
    for name in ("texture_sample", "render_atlas"):
        print(f"wrote {name}.npz, {(HERE / (name + '.npz')).stat().st_size / 1e3:.0f} kB")


if __name__ == "__main__":
    texture_only() if sys.argv[1:] == ["texture_sample"] else main()
