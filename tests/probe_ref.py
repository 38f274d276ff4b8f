"""A numpy restatement of include/terra_amd.h "Probe harmonics", rules of the projection and of the irradiance: binary64 in the stated order (numpy's float64 +, -, *, /
and sqrt are the IEEE operations, and nothing here is fused), np.float32 for the final roundings. The 64 lanes of the projection and the queries of the irradiance are
array axes; every sum along the stated order is a loop. The rays need no restatement: terra_amd_probe_rays is pinned onto terra_amd_unit_point_rays."""
import numpy as np

from terra_amd import api

D, F = np.float64, np.float32
FOUR_PI = D(12.566370614359172)
A = [D(3.141592653589793)] + [D(2.0943951023931953)] * 3 + [D(0.7853981633974483)] * 5


def basis(x, y, z):
    """Y_0 .. Y_8 of the direction (x, y, z), float64 arrays of one shape (Y_0 a scalar), used as given"""
    x, y, z = np.asarray(x, D), np.asarray(y, D), np.asarray(z, D)
    return [D(0.28209479177387814),
            D(0.4886025119029199) * y, D(0.4886025119029199) * z, D(0.4886025119029199) * x,
            D(1.0925484305920792) * (x * y), D(1.0925484305920792) * (y * z), D(0.31539156525252005) * ((D(3.0) * (z * z)) - D(1.0)),
            D(1.0925484305920792) * (x * z), D(0.5462742152960396) * ((x * x) - (y * y))]


def contributes(results, rays):
    """[P, K] bool: samples > 0 and the ray active by the ray door's rule"""
    o, d = rays["origin"], rays["direction"]
    active = np.isfinite(o).all(-1) & np.isfinite(d).all(-1) & (d != 0).any(-1)
    return (results["samples"] > 0) & active


def project(results, rays, cells, batch=0, old=None):
    """results [P, K] api.RESULT_DTYPE, rays [P, K] api.RAY_DTYPE, K = cells * cells -> [P] api.PROBE_SH_DTYPE; old: the records a batch > 0 averages into"""
    P, K = results.shape
    assert K == cells * cells and rays.shape == (P, K)
    out = np.zeros(P, api.PROBE_SH_DTYPE)
    ok = contributes(results, rays)
    rounds = -(-K // 64)
    with np.errstate(all="ignore"):
        for p in range(P):
            d = rays["direction"][p].astype(D)
            L = results["acc"][p].astype(D) / np.where(ok[p], results["samples"][p], 1).astype(D)[:, None]
            Y = np.stack([y * np.ones(K) for y in basis(d[:, 0], d[:, 1], d[:, 2])], axis=1)          # [K, 9]
            terms = np.where(ok[p][:, None, None], L[:, None, :] * Y[:, :, None], D(0.0))          # [K, 9, 3]; a cell that does not contribute adds +0
            lanes = np.zeros((rounds * 64, 9, 3), D)
            lanes[:K] = terms
            lanes = lanes.reshape(rounds, 64, 9, 3)
            partial = np.zeros((64, 9, 3), D)
            for r in range(rounds):          # lane l: its cells l, l + 64, ... in ascending order onto +0.0
                partial = partial + lanes[r]
            s = 32
            while s >= 1:
                partial[:s] = partial[:s] + partial[s:2 * s]
                s //= 2
            new = partial[0] * (FOUR_PI / D(K))
            if batch == 0:
                out["c"][p] = new.astype(F)
            else:
                out["c"][p] = (((old["c"][p].astype(D) * D(batch)) + new) / D(batch + 1)).astype(F)
            out["cells"][p] = ok[p].sum()
    return out


def _axis(pos, origin, spacing, count):
    f = (pos.astype(D) - D(F(origin))) / D(F(spacing))
    bad = np.isnan(f)
    f = np.where(bad, D(0.0), f)
    f = np.where(f < 0.0, D(0.0), f)
    f = np.where(f > D(count - 1), D(count - 1), f)
    lo = np.minimum(np.floor(f).astype(np.int64), max(count - 2, 0))
    return bad, lo, np.minimum(lo + 1, count - 1), f - lo.astype(D)


def irradiance(sh, points, grid=None, index=None):
    """sh [P] api.PROBE_SH_DTYPE, points [n] api.POINT_DTYPE, grid = (origin, spacing, (nx, ny, nz)) or None with index [n] -> float32 [n, 4]"""
    n = len(points)
    with np.errstate(all="ignore"):
        nrm = points["normal"].astype(D)
        q = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        ok = np.isfinite(points["normal"]).all(-1) & (q > 0) & np.isfinite(q)
        N = nrm / np.sqrt(np.where(ok, q, D(1.0)))[:, None]
        if grid is None:
            index = np.asarray(index, np.int64)
            inside = (index >= 0) & (index < len(sh))
            ok &= inside
            c = sh["c"][np.where(inside, index, 0)].astype(D) if len(sh) else np.zeros((n, 9, 3), D)
        else:
            origin, spacing, counts = grid
            axes = [_axis(points["position"][:, a], origin[a], spacing[a], counts[a]) for a in range(3)]
            for bad, _, _, _ in axes:
                ok &= ~bad
            c = None
            for corner in range(8):          # (dz, dy, dx) = 000, 001, ... 111
                up = [corner & 1, (corner >> 1) & 1, corner >> 2]          # per axis x, y, z
                w = [np.where(up[a], axes[a][3], D(1.0) - axes[a][3]) for a in range(3)]
                at = [np.where(up[a], axes[a][2], axes[a][1]) for a in range(3)]
                weight = (w[2] * w[1]) * w[0]
                term = weight[:, None, None] * sh["c"][(at[2] * counts[1] + at[1]) * counts[0] + at[0]].astype(D)
                c = term if c is None else c + term
        Y = basis(N[:, 0], N[:, 1], N[:, 2])
        E = None
        for k in range(9):
            term = (A[k] * c[:, k, :]) * (Y[k] * np.ones(n))[:, None]
            E = term if E is None else E + term
        out = np.zeros((n, 4), F)
        out[:, :3] = np.where(ok[:, None], E.astype(F), F(0))
    return out
