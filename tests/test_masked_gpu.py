"""Masked rendering on the device (include/terra_amd.h "Masked rendering"): a masked launch leaves in every active 16 x 16 block the bits the unmasked call over the
same rectangle leaves, and touches nothing else. Frame 112 x 80, rectangle (8, 5, 100, 70): 7 x 5 mask blocks with a partial last row and column, and 64-pixel
launch tiles that hold blocks without a pixel. One unmasked render precedes every comparison, so the prior sample counts that key the streams are non-zero.
Everything is compared bit for bit: there is no tolerance anywhere in this file.

Masked launches exist for LDS-resident scenes only (the decision rule of the feature's A/B: the kernels that key their streams in place lost 0.4 - 0.5 % of the hall
frames to the block lookup, profiles/masked/ab.md). The two scenes that run those kernels -- the Cornell box on the fast tree, the sphere scene on the reference tree
read from global memory -- are refusal tests here: kTerraAmdErrUnsupported, a message, no byte changed."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, scenes

pytestmark = pytest.mark.gpu
FW, FH = 112, 80
RECT = (8, 5, 100, 70)
ROWS, COLS = 5, 7
SENTINEL = 0x5A5A5A5A
ERR_BAD_ARGUMENT = -4
ERR_UNSUPPORTED = -3


@pytest.fixture(scope="module")
def L(amd_lib):
    import torch
    from terra_amd import runtime
    assert torch.cuda.is_available()
    return runtime.load()


def masks():
    """name -> (ROWS, COLS) uint32 words; "non-zero means active": the active words are not all 1"""
    by, bx = np.mgrid[0:ROWS, 0:COLS]
    rng = np.random.default_rng(20261020)
    out = {"zero": np.zeros((ROWS, COLS), np.uint32), "one": np.ones((ROWS, COLS), np.uint32)}
    single = np.zeros((ROWS, COLS), np.uint32); single[2, 3] = 0x80000000
    out["single"] = single
    out["edge"] = ((by == ROWS - 1) | (bx == COLS - 1)).astype(np.uint32) * 7
    out["checker"] = (((bx + by) & 1) == 0).astype(np.uint32) * 0xffffffff
    out["random30"] = (rng.random((ROWS, COLS)) < 0.3).astype(np.uint32)
    assert 0 < out["random30"].sum() < ROWS * COLS
    return out


def block_rect(bx, by):
    """the clipped rectangle of mask block (bx, by), in frame coordinates"""
    x, y, w, h = RECT
    return x + 16 * bx, y + 16 * by, min(16, w - 16 * bx), min(16, h - 16 * by)


def active_pixels(mask):
    """(FH, FW) bool: the frame pixels that lie in an active block of the rectangle"""
    a = np.zeros((FH, FW), bool)
    for by in range(ROWS):
        for bx in range(COLS):
            if mask[by, bx]:
                x0, y0, w, h = block_rect(bx, by)
                a[y0:y0 + h, x0:x0 + w] = True
    return a


class Frame:
    """pixels, results and the draw counts of one frame in HBM"""

    def __init__(self, src=None):
        import torch
        from terra_amd import runtime
        self.fb = runtime.DeviceFramebuffer(FW, FH)
        self.calls = torch.full((FW * FH,), SENTINEL, dtype=torch.int32, device="cuda")
        if src is not None:
            self.fb.pixels.copy_(src.fb.pixels); self.fb.results.copy_(src.fb.results); self.calls.copy_(src.calls)

    def host(self):
        return (self.fb.pixels.cpu().numpy().view(np.uint32).reshape(FH, FW, 3), self.fb.results.cpu().numpy().view(np.uint32).reshape(FH, FW, 4),
                self.calls.cpu().numpy().view(np.uint32).reshape(FH, FW))


def dev_mask(m):
    import torch
    return torch.from_numpy(m.astype(np.uint32).view(np.int32).reshape(-1).copy()).cuda()


def check_masked(got, full, prior, mask, what, with_calls=True):
    """active blocks: the unmasked call's bits; everything else: the prior buffers', byte for byte"""
    a = active_pixels(mask)
    for k, name in enumerate(("pixels", "results", "calls")):
        if name == "calls" and not with_calls:
            continue
        g, f, p = got[k], full[k], prior[k]
        assert np.array_equal(g[a], f[a]), f"{what}: {name} of an active block differ from the unmasked call"
        assert np.array_equal(g[~a], p[~a]), f"{what}: {name} outside the active blocks changed"
    if not mask.any():
        for k in range(3):
            assert np.array_equal(got[k], prior[k]), f"{what}: the all-zero mask changed something"


def traversal(L, s):
    from terra_amd import runtime
    ti = runtime.TraversalInfo()
    runtime.check(L.traversal_info(s, C.byref(ti)))
    return ti.lds_resident, ti.last_call


SCENES = {
    # name: (description maker, tree_mode, spp by split, (lds_resident, last_call set) expected)
    "cornell": (lambda spp, integ: scenes.cornell_box(FW, FH, spp, integrator=integ), None, {1: 8, 4: 8, 0: 32}, (1, (1, 2))),
    "cornell_fast": (lambda spp, integ: scenes.cornell_box(FW, FH, spp, integrator=integ), 1, {1: 8, 4: 8, 0: 32}, (0, (3, 4))),
    "spheres_ref": (lambda spp, integ: scenes.cornell_spheres(FW, FH, spp, integrator=integ), 0, {1: 2, 4: 2, 0: 2}, (0, (1, 2))),
}


def open_scene(L, name, integ, split, counters=False, job_order=None, pull_back=0.0):
    make, tree_mode, spp_of, _ = SCENES[name]
    d = make(spp_of[split], integ)
    s = scenes.build_scene(L, d, tree_mode=tree_mode, counters=counters)
    assert L.set_sample_split(s, split) == 0
    if job_order is not None:
        assert L.set_job_order(s, job_order) == 0
    cam = scenes.camera_of(d)
    if pull_back:
        cam.position = api.TerraFloat3(cam.position.x - pull_back * cam.direction.x, cam.position.y - pull_back * cam.direction.y, cam.position.z - pull_back * cam.direction.z)
    return s, cam


def run_equalities(L, s, cam, what, expect_pairs=False, with_calls_for=("checker", "random30")):
    """case 1's equalities for every mask: without a draw-count buffer (the launch the library makes by default) and, for some masks, with one"""
    import torch
    from terra_amd import runtime
    prior = Frame()
    runtime.render_device(L, cam, s, prior.fb, rect=RECT)                      # prior samples are non-zero from here on
    full = Frame(prior); runtime.render_device(L, cam, s, full.fb, rect=RECT)
    fullc = Frame(prior); runtime.render_device(L, cam, s, fullc.fb, rect=RECT, rand_calls=fullc.calls)
    torch.cuda.synchronize()
    P, F, FC = prior.host(), full.host(), fullc.host()
    assert np.array_equal(F[1], FC[1])                                         # (the counting launch gives the same sums)
    assert (FC[2][RECT[1]:RECT[1] + RECT[3], RECT[0]:RECT[0] + RECT[2]] != SENTINEL).all()
    for name, m in masks().items():
        g = Frame(prior)
        runtime.render_masked_device(L, cam, s, g.fb, dev_mask(m), rect=RECT)
        if expect_pairs:
            assert runtime.leaf_pair_info(L, s)[0], "the masked launch did not take the pair form"
        torch.cuda.synchronize()
        assert runtime.last_error() == ""
        check_masked(g.host(), F, P, m, f"{what} / {name}", with_calls=False)
        assert np.array_equal(g.host()[2], P[2])                               # no draw-count buffer passed: none written
        if name in with_calls_for:
            g = Frame(prior)
            runtime.render_masked_device(L, cam, s, g.fb, dev_mask(m), rect=RECT, rand_calls=g.calls)
            torch.cuda.synchronize()
            check_masked(g.host(), FC, P, m, f"{what} / {name} / draw counts")


@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect])
@pytest.mark.parametrize("split", [1, 4, 0])
@pytest.mark.parametrize("name", ["cornell"])
def test_active_blocks_equal_the_unmasked_call_and_the_rest_is_untouched(L, name, split, integ):
    from terra_amd import runtime
    s, cam = open_scene(L, name, integ, split)
    try:
        run_equalities(L, s, cam, f"{name} split {split} integrator {integ}", expect_pairs=name == "cornell")
        lds, last = traversal(L, s)
        want_lds, want_last = SCENES[name][3]
        assert lds == want_lds and last in want_last, (name, lds, last)
        if name == "cornell":
            assert runtime.leaf_pair_info(L, s)[1] > 0
    finally:
        L.clear_error()
        L.scene_destroy(s)


@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect])
def test_job_order_and_empty_skip_together(L, integ):
    """the classifier runs (job order 2), blocks are proved empty (camera pulled back 8 units), and the mask adds the fourth class"""
    import torch
    from terra_amd import runtime
    s, cam = open_scene(L, "cornell", integ, 4, job_order=2, pull_back=8.0)
    try:
        assert L.get_empty_skip(s) == 1
        fb = runtime.DeviceFramebuffer(FW, FH)
        runtime.render_device(L, cam, s, fb, rect=RECT)
        proved, total = runtime.empty_skip_info(L, s)
        assert 0 < proved < total, (proved, total)
        runtime.render_masked_device(L, cam, s, fb, dev_mask(masks()["checker"]), rect=RECT)
        mproved, mtotal = runtime.empty_skip_info(L, s)
        assert mtotal == total and 0 < mproved < proved, (mproved, proved)       # the proved blocks among the active ones; the masked ones are not counted
        torch.cuda.synchronize()
        run_equalities(L, s, cam, f"job order + empty skip, integrator {integ}", with_calls_for=())
        assert runtime.empty_skip_info(L, s)[0] > 0
    finally:
        L.clear_error()
        L.scene_destroy(s)


@pytest.mark.parametrize("name", ["cornell"])
def test_checkerboard_equals_hand_issued_block_calls(L, name):
    import torch
    from terra_amd import runtime
    s, cam = open_scene(L, name, api.kTerraIntegratorDirect, 4)
    try:
        prior = Frame(); runtime.render_device(L, cam, s, prior.fb, rect=RECT)
        m = masks()["checker"]
        a = Frame(prior); runtime.render_masked_device(L, cam, s, a.fb, dev_mask(m), rect=RECT, rand_calls=a.calls)
        b = Frame(prior)
        for by in range(ROWS):
            for bx in range(COLS):
                if m[by, bx]:
                    runtime.render_device(L, cam, s, b.fb, rect=block_rect(bx, by), rand_calls=b.calls)
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(a.host(), b.host())):
            assert np.array_equal(x, y), ("pixels", "results", "calls")[k]
    finally:
        L.clear_error()
        L.scene_destroy(s)


@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect])
@pytest.mark.parametrize("name", ["cornell_fast", "spheres_ref"])
def test_scenes_that_key_their_streams_in_place_are_refused(L, name, integ):
    """the fast tree and the reference tree read from global memory: every masked call answers kTerraAmdErrUnsupported with a message and touches nothing"""
    import torch
    from terra_amd import runtime
    s, cam = open_scene(L, name, integ, 1)
    try:
        f = Frame(); runtime.render_device(L, cam, s, f.fb, rect=RECT)
        lds, last = traversal(L, s)
        want_lds, want_last = SCENES[name][3]
        assert lds == want_lds and last in want_last, (name, lds, last)                 # the kernel the unmasked call ran
        aov = runtime.DeviceAov(FW, FH); runtime.render_aov_device(L, cam, s, aov, rect=RECT)
        dm = runtime.DeviceMoments(FW, FH)
        torch.cuda.synchronize()
        before = f.host(); aov_before = aov.data.cpu().numpy().copy()
        mask = dev_mask(masks()["checker"])
        x, y, w, h = RECT
        rep = api.TerraAmdAdaptiveReport()
        calls = (lambda: L.render_masked_device(C.byref(cam), s, f.fb.pixels.data_ptr(), f.fb.results.data_ptr(), FW, FH, x, y, w, h, mask.data_ptr(), f.calls.data_ptr(), None),
                 lambda: L.render_aov_masked_device(C.byref(cam), s, aov.data.data_ptr(), FW, FH, x, y, w, h, mask.data_ptr(), None),
                 lambda: L.render_adaptive_masked_device(C.byref(cam), s, f.fb.pixels.data_ptr(), f.fb.results.data_ptr(), dm.data.data_ptr(), aov.data.data_ptr(), FW, FH, x, y, w, h, None, C.byref(rep), None))
        for call in calls:
            L.clear_error()
            assert call() == ERR_UNSUPPORTED
            assert "LDS-resident" in runtime.last_error()
        torch.cuda.synchronize()
        for a, b in zip(before, f.host()):
            assert np.array_equal(a, b)
        assert np.array_equal(aov_before, aov.data.cpu().numpy()) and not dm.data.cpu().numpy().any() and rep.rounds == 0
        lds2, last2 = traversal(L, s)
        assert (lds2, last2) == (lds, last)
    finally:
        L.clear_error(); L.fn("terra_amd_clear_first_error", None, [])()
        L.scene_destroy(s)


def stats(L, s):
    from terra_amd import runtime
    st = runtime.Stats(); runtime.check(L.get_stats(s, C.byref(st)))
    return st.as_dict()


@pytest.mark.parametrize("name", ["cornell"])
def test_one_launch_and_no_work_for_inactive_blocks(L, name):
    import torch
    from terra_amd import runtime
    s, cam = open_scene(L, name, api.kTerraIntegratorDirect, 1, counters=True)
    try:
        prior = Frame(); runtime.render_device(L, cam, s, prior.fb, rect=RECT)
        M = masks()
        before = stats(L, s)
        g = Frame(prior); runtime.render_masked_device(L, cam, s, g.fb, dev_mask(M["zero"]), rect=RECT)
        after = stats(L, s)
        assert after["launches"] == before["launches"] + 1 and after["rays"] == before["rays"], (before, after)
        g = Frame(prior); runtime.render_masked_device(L, cam, s, g.fb, dev_mask(M["single"]), rect=RECT)
        single = stats(L, s)
        assert single["launches"] == after["launches"] + 1
        u = Frame(prior); runtime.render_device(L, cam, s, u.fb, rect=block_rect(3, 2))
        block = stats(L, s)
        print(f"{name}: rays of the single-block mask {single['rays'] - after['rays']}, of the block's own call {block['rays'] - single['rays']}")
        assert single["rays"] - after["rays"] == block["rays"] - single["rays"] > 0
        torch.cuda.synchronize()
        assert np.array_equal(g.host()[1], u.host()[1])
    finally:
        L.clear_error()
        L.scene_destroy(s)


@pytest.mark.parametrize("split", [1, 4, 0])
@pytest.mark.parametrize("name", ["cornell"])
def test_aov_masked(L, name, split):
    import torch
    from terra_amd import runtime
    s, cam = open_scene(L, name, api.kTerraIntegratorDirect, split)
    try:
        prior = runtime.DeviceAov(FW, FH); runtime.render_aov_device(L, cam, s, prior, rect=RECT)
        full = runtime.DeviceAov(FW, FH); full.data.copy_(prior.data); runtime.render_aov_device(L, cam, s, full, rect=RECT)
        torch.cuda.synchronize()
        P = prior.data.cpu().numpy().view(np.uint32).reshape(FH, FW, 12); F = full.data.cpu().numpy().view(np.uint32).reshape(FH, FW, 12)
        assert (prior.host()["samples"][RECT[1]:RECT[1] + RECT[3], RECT[0]:RECT[0] + RECT[2]] > 0).all()
        for mname, m in masks().items():
            g = runtime.DeviceAov(FW, FH); g.data.copy_(prior.data)
            runtime.render_aov_masked_device(L, cam, s, g, dev_mask(m), rect=RECT)
            torch.cuda.synchronize()
            G = g.data.cpu().numpy().view(np.uint32).reshape(FH, FW, 12)
            a = active_pixels(m)
            assert np.array_equal(G[a], F[a]), (name, split, mname)
            assert np.array_equal(G[~a], P[~a]), (name, split, mname)              # `samples` included
            if not m.any():
                assert np.array_equal(G, P)
    finally:
        L.clear_error()
        L.scene_destroy(s)


@pytest.mark.parametrize("all_", [0, 1])
def test_error_mask_against_numpy(L, all_):
    import torch
    from terra_amd import runtime
    w, h, tile, target = 100, 70, 32, np.float32(0.25)
    tx, ty = -(-w // tile), -(-h // tile)
    err = np.array([np.nan, np.inf, target, np.nextafter(target, np.float32(1)), np.nextafter(target, np.float32(0)), 0.0, -np.inf, 1e30, -0.0, 0.2500001, 3.0, 0.1], np.float32)
    assert err.size == tx * ty
    m = runtime.error_mask_device(L, torch.from_numpy(err).cuda(), w, h, tile=tile, target_error=float(target), all=bool(all_))
    torch.cuda.synchronize()
    got = m.cpu().numpy()
    assert got.shape == (ROWS, COLS)
    want = np.zeros((ROWS, COLS), np.int32)
    for by in range(ROWS):
        for bx in range(COLS):
            e = err[(16 * by // tile) * tx + 16 * bx // tile]
            want[by, bx] = 1 if (all_ or e > target) else 0
    assert np.array_equal(got, want), (got, want)
    if not all_:
        assert want[0, 0] == 0 and want[0, 2] == 1 and want[0, 4] == 0 and want[0, 6] == 1      # NaN, +inf, equality, just above


@pytest.mark.parametrize("pull_back", [0.0, 8.0])
def test_adaptive_masked_equals_the_tile_driver(L, pull_back):
    """pull_back 0: the parameters of tests/test_adaptive.py; 8: its camera moved back, so that the outer tiles stop at min_batches and the later masks are sparse"""
    import torch
    from terra_amd import runtime
    W = H_ = 256
    TILE, SPP, MIN_B, MAX_B, TARGET = 64, 2, 3, 12, 0.06
    d = scenes.cornell_box(W, H_, SPP, integrator=api.kTerraIntegratorDirect)
    s = scenes.build_scene(L, d, counters=False)
    try:
        assert L.set_sample_split(s, 2) == 0
        cam = scenes.camera_of(d)
        cam.position = api.TerraFloat3(cam.position.x - pull_back * cam.direction.x, cam.position.y - pull_back * cam.direction.y, cam.position.z - pull_back * cam.direction.z)
        out = []
        for masked in (False, True):
            fb, dm, aov = runtime.DeviceFramebuffer(W, H_), runtime.DeviceMoments(W, H_), runtime.DeviceAov(W, H_)
            before = stats(L, s)["launches"]
            rep = runtime.render_adaptive_device(L, cam, s, fb, dm, aov, tile=TILE, min_batches=MIN_B, max_batches=MAX_B, target_error=TARGET, masked=masked)
            torch.cuda.synchronize()
            out.append((rep, stats(L, s)["launches"] - before, [t.cpu().numpy().view(np.uint32) for t in (fb.pixels, fb.results, dm.data, aov.data)]))
        (rep_t, launches_t, bufs_t), (rep_m, launches_m, bufs_m) = out
        print("tile driver:", rep_t, launches_t, "launches; masked driver:", rep_m, launches_m, "launches")
        assert rep_m == rep_t
        if pull_back:
            assert rep_t["rounds"] > MIN_B and rep_t["tile_calls"] < rep_t["tiles"] * rep_t["rounds"]      # (tiles did stop early: the later masks were not all ones)
        for a, b, what in zip(bufs_t, bufs_m, ("pixels", "results", "moments", "aov")):
            assert np.array_equal(a, b), what
        assert launches_t == rep_t["tile_calls"] and launches_m == rep_m["rounds"] and launches_m < launches_t
    finally:
        L.clear_error()
        L.scene_destroy(s)


def test_refusals_leave_the_buffers_alone(L):
    import torch
    from terra_amd import runtime
    s, cam = open_scene(L, "cornell", api.kTerraIntegratorDirect, 1)
    try:
        f = Frame(); runtime.render_device(L, cam, s, f.fb, rect=RECT)
        aov = runtime.DeviceAov(FW, FH); runtime.render_aov_device(L, cam, s, aov, rect=RECT)
        torch.cuda.synchronize()
        before = f.host(); aov_before = aov.data.cpu().numpy().copy()
        mask = torch.ones(ROWS * COLS + 1, dtype=torch.int32, device="cuda")
        x, y, w, h = RECT
        pix, res, calls = f.fb.pixels.data_ptr(), f.fb.results.data_ptr(), f.calls.data_ptr()
        beyond = (x, y, FW - x + 1, h)
        for bad_mask, rect in ((None, RECT), (mask.data_ptr() + 1, RECT), (mask.data_ptr() + 2, RECT), (mask.data_ptr(), beyond)):
            L.clear_error()
            rc = L.render_masked_device(C.byref(cam), s, pix, res, FW, FH, *rect, bad_mask, calls, None)
            assert rc == ERR_BAD_ARGUMENT and runtime.last_error() != "", (bad_mask, rect)
            L.clear_error()
            rc = L.render_aov_masked_device(C.byref(cam), s, aov.data.data_ptr(), FW, FH, *rect, bad_mask, None)
            assert rc == ERR_BAD_ARGUMENT and runtime.last_error() != "", (bad_mask, rect)
        L.clear_error()
        assert L.render_device(C.byref(cam), s, pix, res, FW, FH, *beyond, calls, None) == ERR_BAD_ARGUMENT      # the camera call's own code for that rectangle
        L.clear_error()
        assert L.render_masked_device(C.byref(cam), s, None, res, FW, FH, *RECT, mask.data_ptr(), None, None) == L.render_device(C.byref(cam), s, None, res, FW, FH, *RECT, None, None) == ERR_BAD_ARGUMENT
        torch.cuda.synchronize()
        for a, b in zip(before, f.host()):
            assert np.array_equal(a, b)
        assert np.array_equal(aov_before, aov.data.cpu().numpy())
        assert (mask.cpu().numpy() == 1).all()
    finally:
        L.clear_error(); L.fn("terra_amd_clear_first_error", None, [])()
        L.scene_destroy(s)
