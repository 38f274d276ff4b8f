"""the flat leaf-box test where it is dearest: a 32-triangle soup (32 distinct leaf boxes) at 1080p, 64 spp, switch on against off, through
terra_amd_render_device (event-timed, alternated); the Cornell frame (16 boxes) at the same size beside it"""
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch
import harness as H
from terra_amd import api, runtime, scenes
from test_oracle_vs_reference import soup_scene
L = runtime.load()
out = {}
for name in ("soup32", "cornell"):
    d = soup_scene(H, 32, 18, n_objects=3) if name == "soup32" else scenes.cornell_box(1920, 1080, 64)
    d.width, d.height, d.spp = 1920, 1080, 64
    scene = scenes.build_scene(L, d, counters=False); cam = scenes.camera_of(d)
    fb = runtime.DeviceFramebuffer(d.width, d.height)
    res = {"off": [], "on": []}
    for rep in range(4):
        for on in (0, 1):
            runtime.check(L.set_leaf_box_test(scene, on))
            ms = C.c_float(0)
            runtime.check(L.time_render_device(C.byref(cam), scene, fb.pixels.data_ptr(), fb.results.data_ptr(), d.width, d.height, 0, 0, d.width, d.height, 1 if rep == 0 else 3, None, C.byref(ms)))
            if rep:
                res["on" if on else "off"].append(round(ms.value, 4))
            if on:
                res["flat_used_boxes"] = runtime.leaf_box_info(L, scene)
    out[name] = res
print(json.dumps(out))
