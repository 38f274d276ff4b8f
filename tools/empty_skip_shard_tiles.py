"""a 1/8 shard of the headline frame (each of the 8 ranks' launches, event-timed, one GPU) and the 135-tile host loop (128-pixel tiles, 8 threads, terra_render)"""
import ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from terra_amd import api, runtime, scenes
from concurrent.futures import ThreadPoolExecutor
L = runtime.load()
d = scenes.cornell_box(1920, 1080, 512, bounces=8)
scene = scenes.build_scene(L, d, counters=False); cam = scenes.camera_of(d)
runtime.check(L.set_sample_split(scene, 0))
fb = runtime.DeviceFramebuffer(d.width, d.height)
out = {"shard_ms": [], "shard_proved_total": []}
for rank in range(8):
    runtime.render_device_sharded(L, cam, scene, fb, 64, rank, 8); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        runtime.render_device_sharded(L, cam, scene, fb, 64, rank, 8)
    e1.record(); torch.cuda.synchronize()
    out["shard_ms"].append(round(e0.elapsed_time(e1) / 5, 4))
    if L.has("terra_amd_empty_skip_info"):
        out["shard_proved_total"].append(runtime.empty_skip_info(L, scene))
out["shard_slowest_ms"] = max(out["shard_ms"]); out["shard_mean_ms"] = round(sum(out["shard_ms"]) / 8, 4)
hfb = api.Framebuffer(L, d.width, d.height)
tiles = [(x, y, min(128, d.width - x), min(128, d.height - y)) for y in range(0, d.height, 128) for x in range(0, d.width, 128)]
pool = ThreadPoolExecutor(max_workers=8)
def tile_loop():
    def worker(k):
        for t in tiles[k::8]:
            L.render(C.byref(cam), scene, C.byref(hfb.fb), *t)
    list(pool.map(worker, range(8)))
tile_loop()
runs = []
for _ in range(5):
    t = time.perf_counter(); tile_loop(); runs.append(round((time.perf_counter() - t) * 1e3, 3))
pool.shutdown()
assert runtime.last_error() == "", runtime.last_error()
out["tiles"] = len(tiles); out["tile_loop_ms"] = runs; out["tile_loop_ms_mean"] = round(sum(runs) / len(runs), 3)
print(json.dumps(out))
