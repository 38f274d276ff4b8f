"""terra_amd_shade_stage_info: the one check of the launch constants that the first shading stage of the LDS-resident kernels rests on (csrc/dev_types.h
terra_camera_stage_limits, made where a launch's camera is filled in), and its refusals, through the C boundary. Host arithmetic only: no device.
Inside the limits -- aspect * tan ( fov / 2 ) and tan ( fov / 2 ) in [2^-30, 2^20], every entry of the camera's frame at most 2 in magnitude -- a launch
normalises its camera sample and takes its rays' reciprocals without the range tests it cannot fail; outside them it is handed the guarded ray start."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, runtime


@pytest.fixture(scope="module")
def info(amd_lib):
    f = amd_lib.fn("terra_amd_shade_stage_info", C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int)])

    def call(fov=45.0, w=64, h=48, direction=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)):
        cam = api.TerraCamera(); cam.position = api.f3((0.0, 1.0, -3.4)); cam.direction = api.f3(direction); cam.up = api.f3(up); cam.fov = fov
        out = C.c_int(-1)
        rc = f(C.addressof(cam), w, h, C.byref(out))
        return rc, out.value
    call.raw = f
    return call


def tan_half(fov):
    return float(np.tan(np.float64(np.float32(fov) * np.float32(0.0174533)) / 2))          # as the library forms it (src/Terra.c:1794)


def test_ordinary_cameras_take_the_stages(info):
    for fov in (45.0, 60.0, 1.0, 170.0):
        for w, h in ((64, 48), (1920, 1080), (48, 64)):
            assert info(fov, w, h) == (0, 0)
    assert info(45.0, direction=(1.0, 0.06, -0.04)) == (0, 0) and info(45.0, direction=(0.3, -0.9, 0.2), up=(0.0, 0.0, 5.0)) == (0, 0)


def test_limits_of_the_field_of_view(info):
    lo, hi = 1.1e-7, 1e-8
    assert tan_half(lo) >= 2.0 ** -30 > tan_half(hi)
    assert info(lo) == (0, 0) and info(hi) == (0, 1)                      # tan_half_fov on either side of 2^-30
    wide = 179.9999
    assert 2.0 ** 20 < tan_half(wide) < 2.0 ** 22
    assert info(wide) == (0, 1)                                           # tan_half_fov above 2^20
    assert tan_half(179.999) < 2.0 ** 20 and info(179.999, 64, 64) == (0, 0)
    assert tan_half(179.999) * 64 > 2.0 ** 20 and info(179.999, 4096, 64) == (0, 1)          # aspect * tan_half_fov above 2^20 although tan_half_fov is not
    assert tan_half(lo) / 64 < 2.0 ** -30 and info(lo, 64, 4096) == (0, 1)                    # ... and below 2^-30


def test_a_frame_without_a_direction_is_refused_the_stages(info):
    assert info(45.0, direction=(0.0, 0.0, 0.0)) == (0, 1)                # the frame's entries are NaN: no comparison admits them
    assert info(45.0, direction=(0.0, 1.0, 0.0), up=(0.0, 1.0, 0.0)) == (0, 1)          # up along the direction: the x axis has no length
    assert info(float("nan")) == (0, 1)


def test_bad_arguments_fail_with_a_message(info, amd_lib):
    out = C.c_int(-1)
    cam = api.TerraCamera()
    assert info.raw(None, 64, 48, C.byref(out)) != 0 and "terra_amd_shade_stage_info" in runtime.last_error()
    assert info.raw(C.addressof(cam), 64, 48, None) != 0
    assert info.raw(C.addressof(cam), 0, 48, C.byref(out)) != 0 and info.raw(C.addressof(cam), 64, 0, C.byref(out)) != 0
    assert out.value == -1
