"""The two rules of include/terra_amd.h "Lightmap baking" restated in numpy, brute force: the rule of coverage tests EVERY texel against EVERY triangle in binary64 in
the order the header writes it (numpy's float64 arithmetic is IEEE and never fused), so a texel the device's box walk skips shows up; the dilation rule visits the 8
neighbours in the header's order in binary32. Not a test module: tests/test_bake_gpu.py compares the device with these bit for bit."""
import numpy as np

from terra_amd import api

NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))          # (dy, dx), the header's order


def _edge(px, py, ux, uy, vx, vy):
    ex, ey = vx - ux, vy - uy
    t = ((px - ux) * ex + (py - uy) * ey) / (ex * ex + ey * ey)
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    qx, qy = ux + t * ex, uy + t * ey
    return t, (px - qx) * (px - qx) + (py - qy) * (py - qy)


def atlas_points(positions, normals, uvs, width, height, uv_scale=(1.0, 1.0), uv_offset=(0.0, 0.0), margin=0.0):
    """positions, normals [n, 3, 3] float32 (vertex a, b, c), uvs [n, 6] float32 -> (points [height, width, 8] float32, texels [height, width] ATLAS_TEXEL_DTYPE)"""
    positions = np.asarray(positions, np.float32).reshape(-1, 3, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3, 3)
    uvs = np.asarray(uvs, np.float32).reshape(-1, 6)
    sx, sy = (np.float64(np.float32(v)) for v in uv_scale)
    ox, oy = (np.float64(np.float32(v)) for v in uv_offset)
    m = np.float64(np.float32(margin))
    py, px = np.meshgrid(np.arange(height, dtype=np.float64) + 0.5, np.arange(width, dtype=np.float64) + 0.5, indexing="ij")
    best = np.full((height, width), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    best_wb = np.zeros((height, width), np.float64)
    best_wc = np.zeros((height, width), np.float64)
    with np.errstate(all="ignore"):
        for t in range(len(uvs)):
            u = uvs[t].astype(np.float64)
            ax, ay, bx, by, cx, cy = u[0] * sx + ox, u[1] * sy + oy, u[2] * sx + ox, u[3] * sy + oy, u[4] * sx + ox, u[5] * sy + oy
            area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            if not np.all(np.isfinite([ax, ay, bx, by, cx, cy, area2])) or area2 == 0.0:
                continue
            ea = (cx - bx) * (py - by) - (cy - by) * (px - bx)
            eb = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
            ec = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
            inside = ((-ea >= 0.0) & (-eb >= 0.0) & (-ec >= 0.0)) if area2 < 0.0 else ((ea >= 0.0) & (eb >= 0.0) & (ec >= 0.0))
            wb, wc, d2, cand = eb / area2, ec / area2, np.zeros_like(px), inside
            if m > 0.0:
                t0, d0 = _edge(px, py, ax, ay, bx, by)
                t1, d1 = _edge(px, py, bx, by, cx, cy)
                t2, d2c = _edge(px, py, cx, cy, ax, ay)
                owb, owc, od = t0, np.zeros_like(px), d0
                take = d1 < od
                owb, owc, od = np.where(take, 1.0 - t1, owb), np.where(take, t1, owc), np.where(take, d1, od)
                take = d2c < od
                owb, owc, od = np.where(take, 0.0, owb), np.where(take, 1.0 - t2, owc), np.where(take, d2c, od)
                wb, wc, d2 = np.where(inside, wb, owb), np.where(inside, wc, owc), np.where(inside, 0.0, od)
                cand = inside | (od <= m * m)
            key = (d2.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
            win = cand & (key < best)
            best = np.where(win, key, best)
            best_wb = np.where(win, wb, best_wb)
            best_wc = np.where(win, wc, best_wc)
    covered = best != np.uint64(0xFFFFFFFFFFFFFFFF)
    tri = np.where(covered, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), 0)
    wa = (1.0 - best_wb) - best_wc
    points = np.zeros((height, width, 8), np.float32)
    for src, at in ((positions, 0), (normals, 4)):
        v = src[tri].astype(np.float64)          # [h, w, vertex, component]
        mixed = (wa[..., None] * v[..., 0, :] + best_wb[..., None] * v[..., 1, :]) + best_wc[..., None] * v[..., 2, :]
        points[..., at:at + 3] = np.where(covered[..., None], mixed.astype(np.float32), np.float32(0))
    texels = np.zeros((height, width), api.ATLAS_TEXEL_DTYPE)
    texels["triangle"] = np.where(covered, tri, -1)
    texels["wb"] = np.where(covered, best_wb.astype(np.float32), np.float32(0))
    texels["wc"] = np.where(covered, best_wc.astype(np.float32), np.float32(0))
    texels["distance2"] = np.where(covered, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
    return points, texels


def dilate(data, valid, passes):
    """data [height, width, channels] float32, valid [height, width] int32 -> (data, valid) after `passes` passes; the inputs are left as they are"""
    data = np.array(data, np.float32, copy=True)
    valid = np.array(valid, np.int32, copy=True)
    h, w, ch = data.shape
    with np.errstate(all="ignore"):
        for _ in range(passes):
            ok = np.zeros((h + 2, w + 2), bool); ok[1:-1, 1:-1] = valid != 0
            val = np.zeros((h + 2, w + 2, ch), np.float32); val[1:-1, 1:-1] = data
            total = np.zeros((h, w, ch), np.float32)
            count = np.zeros((h, w), np.int32)
            for dy, dx in NEIGHBOURS:
                n_ok = ok[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                n_val = val[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                total = np.where(n_ok[..., None], np.where((count == 0)[..., None], n_val, total + n_val), total)
                count = count + n_ok
            grow = (valid == 0) & (count > 0)
            mean = total / np.maximum(count, 1).astype(np.float32)[..., None]
            data = np.where(grow[..., None], mean, data)
            valid = np.where(grow, np.int32(1), valid)
    return data, valid
