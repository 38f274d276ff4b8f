"""The order in which the sixteen render entry points refuse a call (DESIGN.md "The doors on the host"): four doors -- the pinhole camera, a client's rays, a camera
model, a client's points -- times four forms -- device, host, AOV device, AOV host --, each run on a 4 x 4 frame against every case below that names something the
door takes. Which refusal wins is observable through the status code, most of all on a host without a GPU, where "scene has no device replica" competes with "bad
argument". TABLE holds the status of every (case, entry point), written out: first column a host without a device, second column a host with one. It was recorded
from a build of the commit before the doors' host side was folded (record() below, run against that library), not from the code under test.
Every case is refused before a pointer is followed, so the device forms get host addresses and no kernel runs."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, runtime, scenes

OK_RECT = (0, 0, 4, 4)
PAST_RIGHT = (1, 0, 4, 4)
DOORS = ("camera", "rays", "lens", "points")
FORMS = ("device", "host", "aov_device", "aov_host")
ENTRIES = tuple((d, f) for d in DOORS for f in FORMS)          # the order of a TABLE row
# what a case changes about an otherwise good call, and the doors that take it
ASPECTS = {"uncommitted": DOORS, "null_out": DOORS, "rect": DOORS, "null_records": ("rays", "points"), "odd_records": ("rays", "points"),
           "null_camera": ("camera", "lens"), "bad_lens": ("lens",), "bad_sampling": ("points",)}
SINGLES = {"null framebuffer or AOV": dict(null_out=True), "null records": dict(null_records=True), "records 4 bytes off": dict(odd_records=True),
           "empty width": dict(rect=(0, 0, 0, 4)), "empty height": dict(rect=(0, 0, 4, 0)), "past the right edge": dict(rect=PAST_RIGHT), "past the bottom edge": dict(rect=(0, 2, 4, 3)),
           "null camera": dict(null_camera=True), "bad lens": dict(bad_lens=True), "bad sampling": dict(bad_sampling=True)}
PAIRS = {"bad lens + bad rectangle": dict(bad_lens=True, rect=PAST_RIGHT), "bad sampling + null points": dict(bad_sampling=True, null_records=True),
         "null records + bad rectangle": dict(null_records=True, rect=PAST_RIGHT), "null framebuffer + bad rectangle": dict(null_out=True, rect=PAST_RIGHT),
         "null framebuffer + bad lens": dict(null_out=True, bad_lens=True), "null framebuffer + bad sampling": dict(null_out=True, bad_sampling=True)}
CASES = {"uncommitted": dict(uncommitted=True), **SINGLES, **PAIRS, **{"uncommitted + " + name: dict(uncommitted=True, **kw) for name, kw in {**SINGLES, **PAIRS}.items()}}


def applies(case, door):
    """a case is run against a door that takes everything the case changes: so every call of the matrix carries at least one reason to be refused"""
    return all(door in ASPECTS[a] for a in CASES[case])


class Bench:
    """the scenes, buffers and arguments of the matrix; call(case, entry) -> the status the call answered"""

    def __init__(self, lib):
        self.lib = lib
        d = scenes.cornell_box(4, 4, 1)
        lib.clear_error()
        self.committed = scenes.build_scene(lib, d)
        self.uncommitted = lib.scene_create()
        self.cam = scenes.camera_of(d)
        self.fb = api.Framebuffer(lib, 4, 4)
        self.aov = np.zeros((4, 4), runtime.AOV_DTYPE)
        self.raw = np.zeros(16 * 32 + 32, np.uint8)          # 16 records of 32 bytes (direction / normal +y), 16-byte aligned; the same 4 bytes further on
        self.at = (-self.raw.ctypes.data) % 16
        self.raw[self.at:self.at + 16 * 32].view(np.float32).reshape(16, 8)[:, 5] = 1.0
        self.records_before = self.raw.copy()
        self.lens, self.bad_lens = api.Lens(), api.Lens()
        self.bad_lens.model = 4
        self.sampling, self.bad_sampling = api.PointSampling(), api.PointSampling()
        self.bad_sampling.distribution = 2

    def close(self):
        self.lib.clear_error()
        self.lib.clear_first_error()
        self.fb.destroy()
        self.lib.scene_destroy(self.committed)
        self.lib.scene_destroy(self.uncommitted)

    def untouched(self):
        return not self.aov.view(np.uint8).any() and not self.fb.results.view(np.uint8).any() and not self.fb.pixels.view(np.uint32).any() and np.array_equal(self.raw, self.records_before)

    def call(self, case, entry):
        lib, kw, (door, form) = self.lib, CASES[case], entry
        scene = self.uncommitted if kw.get("uncommitted") else self.committed
        x, y, w, h = kw.get("rect", OK_RECT)
        null_out = kw.get("null_out", False)
        records = None if kw.get("null_records") else self.raw.ctypes.data + self.at + (4 if kw.get("odd_records") else 0)
        cam = None if kw.get("null_camera") else C.byref(self.cam)
        lens = C.byref(self.bad_lens if kw.get("bad_lens") else self.lens)
        ps = C.byref(self.bad_sampling if kw.get("bad_sampling") else self.sampling)
        head = {"camera": (cam, scene), "rays": (scene, records), "lens": (cam, lens, scene), "points": (scene, ps, records)}[door]
        name = {"camera": "", "rays": "_rays", "lens": "_lens", "points": "_points"}[door]
        lib.clear_error()
        lib.clear_first_error()
        if form == "device":
            out = (None, None) if null_out else (self.fb.pixels.ctypes.data, self.fb.results.ctypes.data)
            if door == "camera":
                rc = lib.render_device_sharded(*head, *out, 4, 4, x, y, w, h, 64, 0, 1, None, None)
            else:
                rc = getattr(lib, "render" + name + "_device")(*head, *out, 4, 4, x, y, w, h, None, None)
        elif form == "host":
            fb = None if null_out else C.byref(self.fb.fb)
            rc = (lib.render if door == "camera" else getattr(lib, "render" + name))(*head, fb, x, y, w, h)          # (terra_render is void: its status is the first error's)
        else:
            aov = None if null_out else self.aov.ctypes.data
            rc = getattr(lib, "render_aov" + name + ("_device" if form == "aov_device" else ""))(*head, aov, 4, 4, x, y, w, h, *((None,) if form == "aov_device" else ()))
        status, message = runtime.first_error()
        assert (door, form) == ("camera", "host") or rc == status, (case, entry, rc, status)
        assert runtime.last_error() != "" and message != "", (case, entry)
        return status


def record(lib):
    """{case: row of sixteen statuses (None: the case names something the door does not take)}: what fills a column of TABLE, from a build of the parent commit"""
    b = Bench(lib)
    try:
        return {case: tuple(b.call(case, e) if applies(case, e[0]) else None for e in ENTRIES) for case in CASES}
    finally:
        b.close()


_ = None
# case: (host without a device, host with a device); a row holds camera, rays, lens, points x device, host, AOV device, AOV host
TABLE = {
    "uncommitted": ((-2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2),
                    (-2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2)),
    "null framebuffer or AOV": ((-1, -4, -1, -1, -1, -4, -1, -1, -1, -4, -1, -1, -1, -4, -1, -1),
                                (-4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4)),
    "null records": ((_, _, _, _, -1, -1, -1, -1, _, _, _, _, -4, -4, -4, -4),
                     (_, _, _, _, -4, -4, -4, -4, _, _, _, _, -4, -4, -4, -4)),
    "records 4 bytes off": ((_, _, _, _, -1, -1, -1, -1, _, _, _, _, -4, -4, -4, -4),
                            (_, _, _, _, -4, -4, -4, -4, _, _, _, _, -4, -4, -4, -4)),
    "empty width": ((-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -4, -4, -4, -4),
                    (-4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4)),
    "empty height": ((-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -4, -4, -4, -4),
                     (-4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4)),
    "past the right edge": ((-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -4, -4, -4, -4),
                            (-4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4)),
    "past the bottom edge": ((-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -4, -4, -4, -4),
                             (-4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4)),
    "null camera": ((-1, -1, -1, -1, _, _, _, _, -4, -4, -4, -4, _, _, _, _),
                    (-4, -4, -4, -4, _, _, _, _, -4, -4, -4, -4, _, _, _, _)),
    "bad lens": ((_, _, _, _, _, _, _, _, -4, -4, -4, -4, _, _, _, _),
                 (_, _, _, _, _, _, _, _, -4, -4, -4, -4, _, _, _, _)),
    "bad sampling": ((_, _, _, _, _, _, _, _, _, _, _, _, -4, -4, -4, -4),
                     (_, _, _, _, _, _, _, _, _, _, _, _, -4, -4, -4, -4)),
    "bad lens + bad rectangle": ((_, _, _, _, _, _, _, _, -4, -4, -4, -4, _, _, _, _),
                                 (_, _, _, _, _, _, _, _, -4, -4, -4, -4, _, _, _, _)),
    "bad sampling + null points": ((_, _, _, _, _, _, _, _, _, _, _, _, -4, -4, -4, -4),
                                   (_, _, _, _, _, _, _, _, _, _, _, _, -4, -4, -4, -4)),
    "null records + bad rectangle": ((_, _, _, _, -1, -1, -1, -1, _, _, _, _, -4, -4, -4, -4),
                                     (_, _, _, _, -4, -4, -4, -4, _, _, _, _, -4, -4, -4, -4)),
    "null framebuffer + bad rectangle": ((-1, -4, -1, -1, -1, -4, -1, -1, -1, -4, -1, -1, -4, -4, -4, -4),
                                         (-4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4)),
    "null framebuffer + bad lens": ((_, _, _, _, _, _, _, _, -4, -4, -4, -4, _, _, _, _),
                                    (_, _, _, _, _, _, _, _, -4, -4, -4, -4, _, _, _, _)),
    "null framebuffer + bad sampling": ((_, _, _, _, _, _, _, _, _, _, _, _, -4, -4, -4, -4),
                                        (_, _, _, _, _, _, _, _, _, _, _, _, -4, -4, -4, -4)),
    "uncommitted + null framebuffer or AOV": ((-2, -4, -2, -2, -2, -4, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2),
                                              (-2, -4, -2, -2, -2, -4, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2)),
    "uncommitted + null records": ((_, _, _, _, -2, -2, -2, -2, _, _, _, _, -2, -2, -2, -2),
                                   (_, _, _, _, -2, -2, -2, -2, _, _, _, _, -2, -2, -2, -2)),
    "uncommitted + records 4 bytes off": ((_, _, _, _, -2, -2, -2, -2, _, _, _, _, -2, -2, -2, -2),
                                          (_, _, _, _, -2, -2, -2, -2, _, _, _, _, -2, -2, -2, -2)),
    "uncommitted + empty width": ((-2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2),
                                  (-2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2)),
    "uncommitted + empty height": ((-2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2),
                                   (-2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2)),
    "uncommitted + past the right edge": ((-2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2),
                                          (-2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2)),
    "uncommitted + past the bottom edge": ((-2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2),
                                           (-2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2)),
    "uncommitted + null camera": ((-2, -2, -2, -2, _, _, _, _, -2, -2, -2, -2, _, _, _, _),
                                  (-2, -2, -2, -2, _, _, _, _, -2, -2, -2, -2, _, _, _, _)),
    "uncommitted + bad lens": ((_, _, _, _, _, _, _, _, -2, -2, -2, -2, _, _, _, _),
                               (_, _, _, _, _, _, _, _, -2, -2, -2, -2, _, _, _, _)),
    "uncommitted + bad sampling": ((_, _, _, _, _, _, _, _, _, _, _, _, -2, -2, -2, -2),
                                   (_, _, _, _, _, _, _, _, _, _, _, _, -2, -2, -2, -2)),
    "uncommitted + bad lens + bad rectangle": ((_, _, _, _, _, _, _, _, -2, -2, -2, -2, _, _, _, _),
                                               (_, _, _, _, _, _, _, _, -2, -2, -2, -2, _, _, _, _)),
    "uncommitted + bad sampling + null points": ((_, _, _, _, _, _, _, _, _, _, _, _, -2, -2, -2, -2),
                                                 (_, _, _, _, _, _, _, _, _, _, _, _, -2, -2, -2, -2)),
    "uncommitted + null records + bad rectangle": ((_, _, _, _, -2, -2, -2, -2, _, _, _, _, -2, -2, -2, -2),
                                                   (_, _, _, _, -2, -2, -2, -2, _, _, _, _, -2, -2, -2, -2)),
    "uncommitted + null framebuffer + bad rectangle": ((-2, -4, -2, -2, -2, -4, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2),
                                                       (-2, -4, -2, -2, -2, -4, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2)),
    "uncommitted + null framebuffer + bad lens": ((_, _, _, _, _, _, _, _, -2, -2, -2, -2, _, _, _, _),
                                                  (_, _, _, _, _, _, _, _, -2, -2, -2, -2, _, _, _, _)),
    "uncommitted + null framebuffer + bad sampling": ((_, _, _, _, _, _, _, _, _, _, _, _, -2, -2, -2, -2),
                                                      (_, _, _, _, _, _, _, _, _, _, _, _, -2, -2, -2, -2)),
}


def check_column(lib, column):
    assert set(TABLE) == set(CASES)
    b = Bench(lib)
    try:
        for case in CASES:
            want = TABLE[case][column]
            assert len(want) == 16
            for entry, status in zip(ENTRIES, want):
                assert (status is not None) == applies(case, entry[0]), (case, entry)
                if status is None:
                    continue
                assert status < 0, (case, entry)
                assert b.call(case, entry) == status, (case, entry, runtime.last_error())
                assert b.untouched(), (case, entry)
    finally:
        b.close()


def test_refusal_order_on_this_host(amd_lib):
    """without a device (where this test is meant to run) the first column; on a host that has one the same matrix answers the second"""
    lib = runtime.load(need_torch=False)
    check_column(lib, 1 if lib.device_count() > 0 else 0)


@pytest.mark.gpu
def test_refusal_order_with_a_device(amd_lib):
    lib = runtime.load(need_torch=False)
    assert lib.device_count() > 0, runtime.last_error()
    check_column(lib, 1)
