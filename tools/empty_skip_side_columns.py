"""time at stake: the headline frame's empty side columns alone, through terra_amd_render_device (event-timed)"""
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from terra_amd import api, runtime, scenes
L = runtime.load()
d = scenes.cornell_box(1920, 1080, 512, bounces=8)
scene = scenes.build_scene(L, d, counters=False); cam = scenes.camera_of(d)
runtime.check(L.set_sample_split(scene, 32))
fb = runtime.DeviceFramebuffer(d.width, d.height)
out = {}
for name, rect in (("left_0_400", (0, 0, 400, 1080)), ("right_1520_400", (1520, 0, 400, 1080)), ("full", (0, 0, 1920, 1080))):
    ms = C.c_float(0)
    runtime.check(L.time_render_device(C.byref(cam), scene, fb.pixels.data_ptr(), fb.results.data_ptr(), d.width, d.height, *rect, 1, None, C.byref(ms)))   # warm-up
    runtime.check(L.time_render_device(C.byref(cam), scene, fb.pixels.data_ptr(), fb.results.data_ptr(), d.width, d.height, *rect, 3, None, C.byref(ms)))
    out[name] = round(ms.value, 4)
if L.has("terra_amd_empty_skip_info"):
    out["proved_total_full"] = runtime.empty_skip_info(L, scene)
print(json.dumps(out))
