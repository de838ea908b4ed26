"""NumPy oracle of the BaSiC shading model (Peng et al., Nat. Commun. 8:14836, 2017) as this project
states it ("shading"): inexact-ALM low-rank + sparse fit with DCT-domain smoothness and
darkfield estimation, in float64.  It is the checker of ``magnify_amd.shading``; nothing in the package
imports it."""
from __future__ import annotations

import numpy as np
from scipy.fft import dctn, idctn


def dct2(x):
    return dctn(x, norm="ortho")


def idct2(x):
    return idctn(x, norm="ortho")


def shrink(x, t):
    return np.sign(x) * np.maximum(np.abs(x) - t, 0.0)


def area_matrix(src: int, dst: int) -> np.ndarray:
    """(dst, src) weights of the area resample: row i averages [i*src/dst, (i+1)*src/dst), edge pixels
    weighted by the covered fraction (integer overlaps in units of 1/dst, divided by src)."""
    m = np.zeros((dst, src))
    for i in range(dst):
        a, b = i * src, (i + 1) * src
        for s in range(a // dst, min(-(-b // dst), src)):
            ov = min(b, (s + 1) * dst) - max(a, s * dst)
            if ov > 0:
                m[i, s] = ov
    return m / src


def downsample(tiles, w: int) -> np.ndarray:
    """(N, ty, tx) -> (N, w, w) float32 area means, accumulated in float64."""
    tiles = np.asarray(tiles)
    n, ty, tx = tiles.shape
    my, mx = area_matrix(ty, w), area_matrix(tx, w)
    return (my @ tiles.astype(np.float64) @ mx.T).astype(np.float32)


def linear_matrix(src: int, dst: int) -> np.ndarray:
    """(dst, src) weights of the bilinear resample with half-pixel centres, clamped at the edges."""
    m = np.zeros((dst, src))
    scale = src / dst
    for i in range(dst):
        s = (i + 0.5) * scale - 0.5
        i0 = int(np.floor(s))
        f = s - i0
        if i0 < 0:
            i0, f = 0, 0.0
        if i0 >= src - 1:
            i0, f = src - 1, 0.0
        m[i, i0] += 1.0 - f
        if f > 0:
            m[i, i0 + 1] += f
    return m


def upsample(x, ty: int, tx: int) -> np.ndarray:
    w = x.shape[0]
    return linear_matrix(w, ty) @ np.asarray(x, np.float64) @ linear_matrix(w, tx).T


class Consts:
    def __init__(self, D, get_darkfield=True, smoothness_flatfield=1.0, smoothness_darkfield=1.0,
                 max_iterations=500, optimization_tol=1e-6):
        D = np.asarray(D, np.float64)
        n, w, _ = D.shape
        self.n, self.w = n, w
        m = D.mean(0)
        m = m / m.mean()
        s = np.abs(dct2(m)).sum()
        self.lam_f = 0.5 * smoothness_flatfield * s / 400
        self.lam_d = 0.2 * smoothness_darkfield * s / 400
        flat = D.reshape(n, -1)
        self.norm2 = float(np.sqrt(np.linalg.eigvalsh(flat @ flat.T).max()))
        self.normF = float(np.linalg.norm(flat))
        self.b_up = float(D.min())
        self.get_darkfield = get_darkfield
        self.max_iterations = max_iterations
        self.tol = optimization_tol
        self.ent1, self.ent2 = 1.0, 10.0


class State:
    """The ALM state at the start of a pass."""

    def __init__(self, c: Consts):
        n, w = c.n, c.w
        self.W_hat = np.zeros((w, w))
        self.F_w = np.zeros((w, w))
        self.coeff = np.ones(n)
        self.A_off = np.zeros((w, w))
        self.E = np.zeros((n, w, w))
        self.Y = np.zeros((n, w, w))
        self.B1_off = 0.0
        self.mu = 12.5 / c.norm2
        self.mu_bar = 1e7 * self.mu
        self.rho = 1.5
        self.iterations = 0


def alm_step(st: State, D, weight, c: Consts) -> float:
    """One ALM iteration in place; returns ||Z||_F / ||D||_F."""
    D = np.asarray(D, np.float64)
    mu, ent1, ent2 = st.mu, c.ent1, c.ent2
    A = st.F_w[None] * st.coeff[:, None, None] + st.A_off[None]
    st.W_hat = st.W_hat + dct2((D - A - st.E + st.Y / mu).mean(0) / ent1)
    st.W_hat = shrink(st.W_hat, c.lam_f / (ent1 * mu))
    st.F_w = idct2(st.W_hat)
    A = st.F_w[None] * st.coeff[:, None, None] + st.A_off[None]
    st.E = st.E + (D - A - st.E + st.Y / mu) / ent1
    st.E = shrink(st.E, weight / (ent1 * mu))
    R = D - st.E
    mean_a = A.mean()
    st.coeff = np.maximum(R.mean((1, 2)) / mean_a, 0.0)
    if c.get_darkfield:
        v = st.coeff < 1
        if v.any():
            mf = st.F_w.mean()
            hi, lo = st.F_w > mf - 1e-6, st.F_w < mf + 1e-6
            b1c = (R[v][:, hi].mean(1) - R[v][:, lo].mean(1)) / mean_a
            cv = st.coeff[v]
            k = int(v.sum())
            t1, t2, t3, t4 = (cv**2).sum(), cv.sum(), b1c.sum(), (cv * b1c).sum()
            t5 = t2 * t3 - k * t4
            b1 = 0.0 if t5 == 0 else (t1 * t3 - t2 * t4) / t5
            st.B1_off = min(max(b1, 0.0), c.b_up / mf)
            b_off = st.B1_off * mf - st.B1_off * st.F_w
            a1 = R[v].mean(0) - cv.mean() * st.F_w
            a_off = a1 - a1.mean() - b_off
            thr = c.lam_d / (ent2 * mu)
            a_off = idct2(shrink(dct2(a_off), thr))
            st.A_off = shrink(a_off, thr) + b_off
    Z = D - A - st.E
    st.Y = st.Y + mu * Z
    st.mu = min(st.rho * mu, st.mu_bar)
    st.iterations += 1
    return float(np.linalg.norm(Z) / c.normF)


def alm_pass(D, weight, c: Consts) -> State:
    st = State(c)
    while st.iterations < c.max_iterations:
        if alm_step(st, D, weight, c) < c.tol:
            break
    return st


def fit_working(D, get_darkfield=True, smoothness_flatfield=1.0, smoothness_darkfield=1.0, max_iterations=500,
                optimization_tol=1e-6, max_reweight_iterations=10, reweighting_tol=1e-2, epsilon=0.1):
    """D (N, w, w) -> (flat, dark, iterations per pass) on the working grid."""
    D = np.asarray(D, np.float64)
    c = Consts(D, get_darkfield, smoothness_flatfield, smoothness_darkfield, max_iterations, optimization_tol)
    weight = np.ones_like(D)
    flat_last, dark_last = np.ones(D.shape[1:]), np.zeros(D.shape[1:])
    iterations = []
    flat = dark = None
    for _ in range(max_reweight_iterations):
        st = alm_pass(D, weight, c)
        iterations.append(st.iterations)
        a_off = st.A_off + st.B1_off * st.F_w
        xa = st.F_w[None] * st.coeff[:, None, None] + a_off[None]
        mxa = xa.mean(0)
        weight = 1.0 / (np.abs(st.E / mxa) + epsilon)
        weight = weight * (weight.size / weight.sum())
        flat = mxa - a_off
        flat = flat / flat.mean()
        dark = a_off if get_darkfield else np.zeros_like(a_off)
        mad_f = np.abs(flat - flat_last).sum() / np.abs(flat_last).sum()
        dd = np.abs(dark - dark_last).sum()
        mad_d = 0.0 if dd < 1e-7 else dd / max(np.abs(dark_last).sum(), 1e-6)
        flat_last, dark_last = flat, dark
        if max(mad_f, mad_d) <= reweighting_tol:
            break
    return flat, dark, iterations


def full_fields(flat_w, dark_w, ty, tx):
    """Working-grid fields -> (ty, tx) float32 flat (mean 1) and dark."""
    flat = upsample(flat_w, ty, tx)
    flat = flat / flat.mean()
    return flat.astype(np.float32), upsample(dark_w, ty, tx).astype(np.float32)


def fit(tiles, working_size=128, **kw):
    tiles = np.asarray(tiles)
    tiles = tiles.reshape((-1,) + tiles.shape[-2:])
    ty, tx = tiles.shape[-2:]
    w = min(working_size, ty, tx)
    flat_w, dark_w, its = fit_working(downsample(tiles, w), **kw)
    flat, dark = full_fields(flat_w, dark_w, ty, tx)
    return flat, dark, its


def apply(tiles, flat, dark):
    """(x - dark) / flat per pixel in the tile dtype (integer outputs clamped and truncated)."""
    tiles = np.asarray(tiles)
    if tiles.dtype == np.float64:
        v = (tiles - dark.astype(np.float64)) / flat.astype(np.float64)
    else:
        v = (tiles.astype(np.float32) - dark.astype(np.float32)) / flat.astype(np.float32)
    if tiles.dtype.kind == "u":
        v = np.clip(v, 0, np.iinfo(tiles.dtype).max)
    return v.astype(tiles.dtype)


def synthetic_stack(n=32, size=512, seed=0, strength=0.4):
    """uint16 tiles = (per-tile baseline + beads) * flat + dark: flat = synth.vignette(strength) scaled to mean 1,
    a smooth dark of 100-300 counts, baselines 1000 +- 50 %, sparse beads of synth.noisy_bead_image."""
    from synth import noisy_bead_image, vignette

    rng = np.random.default_rng(seed)
    flat = vignette((size, size), strength=strength).astype(np.float64)
    flat /= flat.mean()
    yy, xx = np.mgrid[0:size, 0:size] / size
    dark = 200 + 100 * np.sin(2 * np.pi * (0.6 * xx + 0.3 * yy))
    tiles = []
    for i in range(n):
        img, _ = noisy_bead_image(seed * 1000 + i, (size, size), 6)
        base = 1000 * (1 + rng.uniform(-0.5, 0.5))
        sig = base + img.astype(np.float64) - 100
        tiles.append(np.clip(np.rint(sig * flat + dark), 0, 65535).astype(np.uint16))
    return np.stack(tiles), flat, dark


def recovery(flat, dark, true_flat, true_dark):
    """(max |flat error| over the central 80 %, max |error of dark minus its mean| / dark range over the central 80 %,
    |mean dark error| / dark range)."""
    h, w = true_flat.shape
    c = (slice(h // 10, h - h // 10), slice(w // 10, w - w // 10))
    rng = true_dark.max() - true_dark.min()
    ef = np.abs(flat[c] - true_flat[c]).max()
    d0, t0 = dark[c] - dark[c].mean(), true_dark[c] - true_dark[c].mean()
    return float(ef), float(np.abs(d0 - t0).max() / rng), float(abs(dark[c].mean() - true_dark[c].mean()) / rng)
