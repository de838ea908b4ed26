"""The contract of mg_roi_refine_circles (include/magnify_hip.h) restated in plain NumPy loops: a radial edge search
along K rays about a start circle, then a centred Kasa circle fit with one rejection round.  Everything is float64, one
operation at a time in the order written here -- NumPy scalars round every operation, so there is nothing to contract --
and the kernel equals this bit for bit.  No square root and no trigonometric function: the direction table comes in.

``refine_window`` takes ONE window; ``refine_block`` loops it over (marker, time) with the kernel's layouts."""
from __future__ import annotations

import numpy as np

SUBPIXEL = 16
CENTRE_MIN, CENTRE_MAX = -1024 * SUBPIXEL, 2048 * SUBPIXEL  # mg_roi_radial_profile's clamp
RADIUS_MAX = 1024 * SUBPIXEL
MAX_RAYS, MAX_REACH, MAX_LEN = 128, 8, 1024
OK, TOO_FEW, DEGENERATE, OUT_OF_REACH = 0, 1, 2, 3
f64 = np.float64


def direction_table(rays):
    """double[K][2] = {cos, sin}(2 pi k / K), as the host computes it with NumPy."""
    a = (2.0 * np.pi * np.arange(rays, dtype=np.float64)) / float(rays)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))


def _fit(u, v, idx):
    """Rule 7 over the rays ``idx`` (ascending): (status, a', ..) -> (ok, a, b, R2)."""
    n = f64(len(idx))
    su = sv = f64(0.0)
    for k in idx:
        su = su + u[k]
        sv = sv + v[k]
    mu, mv = su / n, sv / n
    suu = suv = svv = suz = svz = f64(0.0)
    for k in idx:
        du, dv = u[k] - mu, v[k] - mv
        z = du * du + dv * dv
        suu = suu + du * du
        suv = suv + du * dv
        svv = svv + dv * dv
        suz = suz + du * z
        svz = svz + dv * z
    det = suu * svv - suv * suv
    if not det > 0.0:
        return False, f64(0.0), f64(0.0), f64(0.0)
    a1 = (f64(0.5) * (suz * svv - svz * suv)) / det
    b1 = (f64(0.5) * (svz * suu - suz * suv)) / det
    a, b = mu + a1, mv + b1
    r2 = (a1 * a1 + b1 * b1) + (suu + svv) / n
    if not r2 > 0.0:
        return False, a, b, r2
    return True, a, b, r2


def _residual(u, v, k, a, b, r2):
    da, db = u[k] - a, v[k] - b
    return (da * da + db * db) - r2


def refine_window(win, circle_q, cs, reach, polarity, reject, min_strength, min_rays):
    """One window ``win`` (L, L) of uint8 / uint16 / float32 / float64, ``circle_q`` = {cy, cx, r} in 1/16 pixel, ``cs``
    (K, 2) float64.  -> dict: info int32[4] = {status, n_used, n_valid, polarity}, fit float64[5] = {dy, dx, R2, msq,
    mean strength} (NaN where status != 0), rho (K,) and w (K,) -- NaN where the ray is not valid -- and ``kept``, the
    final set."""
    with np.errstate(all="ignore"):
        return _refine_window(win, circle_q, cs, reach, polarity, reject, min_strength, min_rays)


def _refine_window(win, circle_q, cs, reach, polarity, reject, min_strength, min_rays):
    L = win.shape[0]
    K = cs.shape[0]
    J = 4 * reach + 1
    cy = f64(min(max(int(circle_q[0]), CENTRE_MIN), CENTRE_MAX)) / f64(SUBPIXEL)
    cx = f64(min(max(int(circle_q[1]), CENTRE_MIN), CENTRE_MAX)) / f64(SUBPIXEL)
    r = f64(min(max(int(circle_q[2]), 0), RADIUS_MAX)) / f64(SUBPIXEL)
    rho_j = [(r - f64(reach)) + f64(0.5) * f64(j) for j in range(J)]
    j_lo = next(j for j in range(J) if rho_j[j] >= 0.0)
    first, last = j_lo + 1, J - 2  # the derivative indices
    reject, min_strength = f64(reject), f64(min_strength)

    # 1, 2: samples; a ray is usable iff every sample from j_lo on is inside and finite
    val = np.full((K, J), np.nan)
    usable = np.zeros(K, dtype=bool)
    for k in range(K):
        c, s = f64(cs[k, 0]), f64(cs[k, 1])
        ok = True
        for j in range(j_lo, J):
            y = cy + rho_j[j] * s
            x = cx + rho_j[j] * c
            if not (y >= 0.0 and y < f64(L - 1) and x >= 0.0 and x < f64(L - 1)):  # 0 <= floor, floor + 1 <= L - 1
                ok = False
                continue
            fly, flx = np.floor(y), np.floor(x)
            iy, ix = int(fly), int(flx)
            fy, fx = y - fly, x - flx
            w00, w01, w10, w11 = (f64(win[iy, ix]), f64(win[iy, ix + 1]), f64(win[iy + 1, ix]), f64(win[iy + 1, ix + 1]))
            top = w00 * (f64(1.0) - fx) + w01 * fx
            bot = w10 * (f64(1.0) - fx) + w11 * fx
            val[k, j] = top * (f64(1.0) - fy) + bot * fy
            if not np.isfinite(val[k, j]):
                ok = False
        usable[k] = ok

    # 3, 4: derivatives and polarity
    d = np.full((K, J), np.nan)
    for k in range(K):
        if usable[k]:
            for j in range(first, last + 1):
                d[k, j] = val[k, j + 1] - val[k, j - 1]
    if polarity == 0:
        pp = pm = f64(0.0)
        for k in range(K):
            if usable[k]:
                hi, lo = d[k, first], -d[k, first]
                for j in range(first + 1, last + 1):
                    if d[k, j] > hi:
                        hi = d[k, j]
                    if -d[k, j] > lo:
                        lo = -d[k, j]
                pp = pp + hi
                pm = pm + lo
        pol = 1 if pp >= pm else -1
    else:
        pol = 1 if polarity > 0 else -1

    # 5: the edge on every ray
    rho = np.full(K, np.nan)
    w = np.full(K, np.nan)
    valid = np.zeros(K, dtype=bool)
    for k in range(K):
        if not usable[k]:
            continue
        e = f64(pol) * d[k]
        js = first
        for j in range(first + 1, last + 1):
            if e[j] > e[js]:
                js = j
        if not (e[js] > 0.0) or js == first or js == last:
            continue
        em, e0, ep = e[js - 1], e[js], e[js + 1]
        delta = (f64(0.5) * (em - ep)) / ((em - f64(2.0) * e0) + ep)
        rho[k] = rho_j[js] + f64(0.5) * delta
        w[k] = e0
        valid[k] = True
    n_valid = int(valid.sum())

    info = np.array([OK, 0, n_valid, pol], dtype=np.int32)
    out = {"info": info, "fit": np.full(5, np.nan), "rho": rho, "w": w, "kept": np.zeros(K, dtype=bool)}

    # 6: strength gate
    wmax = f64(0.0)
    for k in range(K):
        if valid[k] and w[k] > wmax:
            wmax = w[k]
    gate = min_strength * wmax
    idx = [k for k in range(K) if valid[k] and w[k] >= gate]
    info[1] = len(idx)
    out["kept"][idx] = True
    if len(idx) < min_rays:
        info[0] = TOO_FEW
        return out

    # 7, 8: fit, reject once, refit
    u = rho * cs[:, 0]
    v = rho * cs[:, 1]
    ok, a, b, r2 = _fit(u, v, idx)
    if ok:
        limit = (f64(4.0) * (reject * reject)) * r2
        rest = []
        for k in idx:
            g = _residual(u, v, k, a, b, r2)
            if not g * g > limit:
                rest.append(k)
        if len(rest) < len(idx) and len(rest) >= min_rays:
            idx = rest
            ok, a, b, r2 = _fit(u, v, idx)
    info[1] = len(idx)
    out["kept"][:] = False
    out["kept"][idx] = True
    if not ok:
        info[0] = DEGENERATE
        return out
    n = f64(len(idx))
    sg = sw = f64(0.0)
    for k in idx:
        g = _residual(u, v, k, a, b, r2)
        sg = sg + g * g
        sw = sw + w[k]
    msq = sg / ((f64(4.0) * r2) * n)
    mw = sw / n
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(r2) and np.isfinite(msq) and np.isfinite(mw)):
        info[0] = DEGENERATE
        return out
    # 9: out of reach
    lo = r - f64(reach)
    if lo < 0.0:
        lo = f64(0.0)
    hi = r + f64(reach)
    if a * a + b * b > f64(reach) * f64(reach) or r2 < lo * lo or r2 > hi * hi:
        info[0] = OUT_OF_REACH
        return out
    out["fit"] = np.array([b, a, r2, msq, mw], dtype=np.float64)
    return out


def refine_block(planes, circles_q, cs, reach=3, polarity=0, reject=1.0, min_strength=0.25, min_rays=None):
    """``planes`` (M, T, L, L), ``circles_q`` int (M, 3) or (M, T' in {1, T}, 3) -> info int32 (M, T, 4), fit float64
    (M, T, 5)."""
    planes = np.asarray(planes)
    m, t = planes.shape[:2]
    c = np.asarray(circles_q)
    if c.ndim == 2:
        c = c[:, None]
    min_rays = cs.shape[0] // 2 if min_rays is None else min_rays
    info = np.zeros((m, t, 4), dtype=np.int32)
    fit = np.full((m, t, 5), np.nan)
    for g in range(m):
        for i in range(t):
            o = refine_window(planes[g, i], c[g, i if c.shape[1] > 1 else 0], cs, reach, polarity, reject, min_strength,
                              min_rays)
            info[g, i], fit[g, i] = o["info"], o["fit"]
    return info, fit
