"""The start of a ray on the device, against the oracle, bit for bit: csrc/trace_geometry.h ray_start_masks (the axes as lane predicates, the numbers from perm),
make_ray_guarded's flag answering the traversal entry's range tests and the azimuth fetched by its integer in the kernels of ray_start_masks_for; ray_state_init,
unchanged, everywhere else.

* Every direction of tests/test_ray_start.py -- {+-0, +-denormal, +-1, +-nextafter(1), +-2, +-inf, NaN}^3 -- from three origins inside the Cornell box (32
  triangles): through terra_amd_unit_watertight_pair at the box's own quads, whose kernel starts its ray with make_ray_guarded and ray_start_masks -- every tie,
  infinity and NaN goes through the predicate form, the origin it picks and the ix / iy / iz it takes from perm's tables -- and through
  terra_amd_intersect_device in the three tree modes (the integer form's entries: they must stay what they were). One launch takes the directions as listed:
  the last component runs through all thirteen values within thirteen rays, so every wave holds lanes that the guard turns away. One launch takes only the
  directions of {+-1, +-nextafter(1), +-2}^3: every lane passes the guard.
* Frames: Cornell at 64 x 64, 4 spp, 8 bounces under Simple and Direct -- the predicate form, the one range test (nearly every wave is all guarded) and the
  azimuth index, closest hits and shadow rays, the pair form behind the flat leaf-box loop; the same at 65 x 65 without jitter, where waves hold rays the guard
  turns away; a 32-triangle soup (the single form: perm and the ranked copies) and a 200-triangle scene (the fast tree) at 32 x 32."""
import numpy as np
import pytest

from terra_amd import api, runtime, scenes
from test_oracle_vs_reference import soup_scene
from test_flat_loop_layout_gpu import oracle as oracle_frame, equals_oracle
from test_leaf_pairs_gpu import dev, _unit
from test_ray_query import pack, to_device
from test_ray_start import directions, xd_rcp_ok

pytestmark = pytest.mark.gpu
ORIGINS = np.array([(0.0, 1.0, 0.0), (-0.55, 0.35, -0.6), (0.7, 1.6, -0.4)], np.float32)          # in the room, outside its two boxes
MODES = [0, 1, 2]


@pytest.fixture(scope="module")
def G(amd_lib):
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def cornell():
    return scenes.cornell_box(16, 16, 1)


def rays_of(d):
    return np.ascontiguousarray(np.repeat(ORIGINS, len(d), axis=0)), np.ascontiguousarray(np.tile(d, (len(ORIGINS), 1)))


@pytest.fixture(scope="module")
def cases(H, orc_lib):
    """both ray sets with the oracle's traversal of them and its watertight test of each ray against the two triangles of a quad of the box, computed once"""
    d_all = directions()
    guarded = xd_rcp_ok(d_all).all(axis=1)
    assert guarded.sum() == 6 ** 3
    ok = np.tile(guarded, len(ORIGINS))                                  # (the order of rays_of)
    assert all(not ok[w:w + 64].all() for w in range(0, len(ok), 64))
    tris = np.concatenate([np.asarray(ob.triangles, np.float32).reshape(-1, 3, 3) for ob in cornell().objects])
    assert len(tris) == 32
    u = H.Unit("orc")
    sc = scenes.build_scene(u.L, cornell())
    out = {}
    for name, d in (("as-listed", d_all), ("guarded-only", d_all[guarded])):
        o, dd = rays_of(d)
        found, prim, point = u.bvh_traverse(sc, o, dd)
        k = (np.arange(len(o)) % 16) * 2                                 # ray i meets quad i mod 16: triangles 2 k, 2 k + 1 = (p0 p1 p2), (p0 p2 p3)
        t1, t2 = tris[k], tris[k + 1]
        assert np.array_equal(t1[:, 0], t2[:, 0]) and np.array_equal(t1[:, 2], t2[:, 1])
        single = [u.watertight(o, dd, np.ascontiguousarray(t.reshape(-1, 9))) for t in (t1, t2)]
        quads = np.ascontiguousarray(np.concatenate([t1, t2[:, 2:]], axis=1).reshape(-1, 12))
        out[name] = dict(o=o, d=dd, found=found, prim=prim, point=point, single=single, quads=quads)
    u.L.scene_destroy(sc)
    assert (out["as-listed"]["found"] != 0).sum() > 500 and (out["guarded-only"]["found"] != 0).sum() > 300      # (the room is open towards -z)
    return out


def same_bits_or_nan(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["as-listed", "guarded-only"])
def test_closest_hits_of_every_direction(G, cases, name, mode):
    c = cases[name]
    G.clear_error()
    scene = scenes.build_scene(G, cornell(), tree_mode=mode)
    assert runtime.last_error() == "", runtime.last_error()
    try:
        t = to_device(pack(c["o"], c["d"], np.float32(np.inf)))
        hits = runtime.intersect(G, scene, t).cpu().numpy().view(api.HIT_DTYPE).reshape(-1)
        occ = runtime.occluded(G, scene, t).cpu().numpy()
    finally:
        G.scene_destroy(scene)
    hit = c["found"] != 0
    assert np.array_equal(hit, hits["object"] >= 0) and np.array_equal(occ, hit.astype(np.int32))
    assert np.array_equal(hits["object"][hit].astype(np.int64), (c["prim"][hit] & 0xff).astype(np.int64))
    assert np.array_equal(hits["triangle"][hit].astype(np.int64), (c["prim"][hit] >> 8).astype(np.int64))
    assert same_bits_or_nan(hits["point"][hit], c["point"][hit])         # (a NaN's payload is the processor's: inf * 0 of a hit at depth 0)


@pytest.mark.parametrize("name", ["as-listed", "guarded-only"])
def test_pair_test_of_every_direction(G, cases, name):
    c = cases[name]
    n = len(c["o"])
    hp, dp = _unit(G, "terra_amd_unit_watertight_pair", n, c["o"], c["d"], c["quads"], (2, 2))
    hits = 0
    for k, (h, out) in enumerate(c["single"]):
        # A direction with a NaN shear (a zero or infinite d[iz], a NaN component) makes every edge function a NaN: no comparison of the test rejects it and the
        # single test "hits" at a NaN depth -- a hit no traversal records, since a NaN depth is below no record. The pair form takes T2's diagonal edge function
        # as -V1, which for a NaN differs in the sign bit alone, so its sign test may drop such a T2. What is held: every hit at a depth that is a number, flag
        # and depth bit for bit; and no number where the oracle has a NaN.
        nan = (h == 1) & np.isnan(out[:, 3])
        assert np.array_equal(hp[~nan, k], h[~nan]), (k, int((hp[~nan, k] != h[~nan]).sum()))
        on = (h == 1) & ~nan
        assert np.array_equal(dp[on, k].view(np.uint32), out[on, 3].view(np.uint32)), k
        assert np.isnan(dp[nan & (hp[:, k] == 1), k]).all(), k
        hits += int(on.sum())
    assert hits > (100 if name == "as-listed" else 30)


@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect], ids=["simple", "direct"])
def test_cornell_frame(G, H, orc_lib, integ):
    mk = lambda: scenes.cornell_box(64, 64, 4, bounces=8, integrator=integ)
    got = dev(G, mk(), 1)
    assert got["used"] and got["flat"] and got["n_pairs"] == 16 and (got["samples"] == 4).all() and got["acc"].sum() > 0
    assert equals_oracle(got, oracle_frame(H, mk()))


@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect], ids=["simple", "direct"])
def test_cornell_frame_with_rays_the_guard_turns_away(G, H, orc_lib, integ):
    """65 x 65 without jitter: the film position of the middle column and of the middle row is exactly 0, so those camera rays have a zero component (the default
    camera looks along +z unrotated), make_ray's guard fails in their lanes and their waves are decided by the range tests on the reciprocals, as before"""
    mk = lambda: scenes.cornell_box(65, 65, 4, bounces=8, integrator=integ, jitter=0.0)
    got = dev(G, mk(), 1)
    assert got["used"] and got["flat"] and (got["samples"] == 4).all() and got["acc"].sum() > 0
    assert equals_oracle(got, oracle_frame(H, mk()))


def small_scene(H, n):
    d = soup_scene(H, n, 40 + n)
    d.width, d.height, d.spp, d.bounces = 32, 32, 4, 8
    return d


@pytest.mark.parametrize("n", [32, 200], ids=["soup-32-single-form", "soup-200-fast-tree"])
def test_soup_frame(G, H, orc_lib, n):
    got = dev(G, small_scene(H, n), 1)
    assert not got["used"] and got["flat"] == (n == 32)                  # no pairs in a soup; 32 triangles are LDS-resident behind the flat loop, 200 take the fast tree
    assert got["acc"].sum() > 0 and equals_oracle(got, oracle_frame(H, small_scene(H, n)))
