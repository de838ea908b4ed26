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


# ---- the mirrored, staged restatement -------------------------------------------------------------------------------
# The functions above state the model.  Those below restate what the HIP kernels (csrc/mg_shading.hip, mg_shadeop.h)
# compute, stage by stage, in np.longdouble, with a float32 rounding exactly where a kernel stores one (the working
# stack, E, Y, the weights, the full-grid fields).  Each stage can take its inputs from the device, so a comparison
# isolates that stage's own rounding: tests/test_gpu_shading_stages.py.

LD = np.longdouble
ENT1, ENT2, RHO = 1.0, 10.0, 1.5
EPS_HI_LO = 1e-6  # the hi / lo pixel classes of the offset regression: fw > mean(F_w) - 1e-6, fw < mean(F_w) + 1e-6


def overlap_matrix(src: int, dst: int) -> np.ndarray:
    """(dst, src) int64 overlaps of the area resample in units of 1 / dst; every row sums to src."""
    m = np.zeros((dst, src), np.int64)
    for i in range(dst):
        a, b = i * src, (i + 1) * src
        for s in range(a // dst, min(-(-b // dst), src)):
            m[i, s] = max(min(b, (s + 1) * dst) - max(a, s * dst), 0)
    return m


def downsample_exact(tiles, w: int) -> np.ndarray:
    """(N, ty, tx) -> (N, w, w) float32 as k_downsample rounds it: the weighted sum S exactly for integer tiles
    (S <= 65535 ty tx < 2^53, so the kernel's float64 sums are exact), then float32(float64(S) / float64(ty tx));
    for float tiles the sums in longdouble."""
    tiles = np.asarray(tiles)
    n, ty, tx = tiles.shape
    oy, ox = overlap_matrix(ty, w), overlap_matrix(tx, w)
    if tiles.dtype.kind in "iu":
        s = oy @ tiles.astype(np.int64) @ ox.T
        assert int(s.max(initial=0)) < 2**53
        return (s.astype(np.float64) / np.float64(ty * tx)).astype(np.float32)
    s = oy.astype(LD) @ tiles.astype(LD) @ ox.T.astype(LD)
    return (s / LD(ty * tx)).astype(np.float32)


def _pi_ld():
    return LD(4) * np.arctan(LD(1))


def cos_table(w: int) -> np.ndarray:
    """Orthonormal DCT-II table C[k][x] = a_k cos(pi (2x+1) k / (2w)) in longdouble (argument reduced exactly)."""
    k, x = np.mgrid[0:w, 0:w]
    r = ((2 * x + 1) * k) % (4 * w)
    a = np.where(k == 0, np.sqrt(LD(1) / w), np.sqrt(LD(2) / w))
    return a * np.cos(_pi_ld() * r.astype(LD) / LD(2 * w))


def cos_table_bound(w: int) -> np.ndarray:
    """Per-entry bound on a float64 table made as a_k * cos(M_PI * (2x+1)k / (2w)): the argument theta carries two
    roundings (product, quotient) of 2^-53 theta each plus that of M_PI, and |cos'| <= 1: 2^-51 theta; cos, sqrt,
    the division under it and the product a_k * cos add less than 2^-51 relative; all scaled by a_k."""
    k, x = np.mgrid[0:w, 0:w]
    theta = np.pi * ((2 * x + 1) * k) / (2.0 * w)
    a = np.where(k == 0, np.sqrt(1.0 / w), np.sqrt(2.0 / w))
    return a * (2.0**-51 * theta + 2.0**-51)


def shrink_ld(x, t):
    return np.where(x > t, x - t, np.where(x < -t, x + t, LD(0)))


def state_dict(st: State) -> dict:
    """The oracle's State as the dictionary alm_stages starts from."""
    return dict(What=st.W_hat, Fw=st.F_w, Aoff=st.A_off, coeff=st.coeff, E=st.E, Y=st.Y, B1=st.B1_off, mu=st.mu,
                mu_bar=st.mu_bar, iterations=st.iterations, cbar=0.0, meanA1=0.0,
                M=np.zeros_like(st.F_w))


def alm_stages(state0: dict, D, weight, consts, get_darkfield, dev=None, round32=True, table=None) -> dict:
    """Every observable value of one ALM iteration as mg_shading_alm_iterate computes it, in longdouble.

    state0: What, Fw, Aoff, coeff, E, Y, B1, cbar, meanA1, mu, mu_bar, iterations at the start of the iteration;
    consts: lam_f, lam_d, normF, b_up, tol, max_iterations.  ``dev`` maps a name of the result to the device's value:
    where given, the stages that consume that value read the device's, so each stage is checked from its own inputs,
    and the discrete decisions (hi / lo, coeff < 1, t5 == 0) are taken in float64 with the kernel's expressions.
    round32: E and Y rounded to float32 as k_update stores them (off: the model in extended precision)."""
    dev = dev or {}

    def f64(x):
        return np.asarray(x).astype(np.float64)

    def take(name, value):
        out[name] = value
        return np.asarray(dev[name]).astype(LD) if name in dev else value

    out = {}
    D = np.asarray(D).astype(LD)
    n, w, _ = D.shape
    P = w * w
    C = np.asarray(table).astype(LD) if table is not None else cos_table(w)
    mu = LD(state0["mu"])
    Fw0, Aoff0, What0 = (np.asarray(state0[k]).astype(LD) for k in ("Fw", "Aoff", "What"))
    coeff0 = np.asarray(state0["coeff"]).astype(LD)
    E0, Y0 = np.asarray(state0["E"]).astype(LD), np.asarray(state0["Y"]).astype(LD)
    wt = np.asarray(weight).astype(LD)

    # k_resid_mean
    A0 = Fw0[None] * coeff0[:, None, None] + Aoff0[None]
    M = take("M", (((D - A0) - E0) + Y0 / mu).sum(0) / n / ENT1)
    # k_mm x 2, MM_WHAT
    What = take("What", shrink_ld(What0 + C @ M @ C.T, LD(consts.lam_f) / (ENT1 * mu)))
    # k_mm x 2, MM_FW
    Fw = take("Fw", C.T @ What @ C)
    meanF = take("meanF", Fw.sum() / P)
    if "Fw" in dev:
        hi = f64(dev["Fw"]) > f64(dev.get("meanF", f64(meanF))) - EPS_HI_LO
        lo = f64(dev["Fw"]) < f64(dev.get("meanF", f64(meanF))) + EPS_HI_LO
    else:
        hi, lo = Fw > meanF - EPS_HI_LO, Fw < meanF + EPS_HI_LO
    # k_update
    A = Fw[None] * coeff0[:, None, None] + Aoff0[None]
    thr_e = wt / (ENT1 * mu)
    pre = E0 + (((D - A) - E0) + Y0 / mu) / ENT1
    e_ld = shrink_ld(pre, thr_e)
    out["E_pre"], out["E_thr"], out["E_ld"] = pre, thr_e, e_ld
    E = take("E", e_ld.astype(np.float32).astype(LD) if round32 else e_ld)
    R = D - E
    Z = (D - A) - E
    y_ld = Y0 + mu * Z
    out["Y_ld"] = y_ld
    Y = take("Y", y_ld.astype(np.float32).astype(LD) if round32 else y_ld)
    tot = np.stack([R.sum((1, 2)), (R * hi).sum((1, 2)), (R * lo).sum((1, 2)), A.sum((1, 2)), (Z * Z).sum((1, 2)),
                    np.full(n, LD(hi.sum())), np.full(n, LD(lo.sum()))], axis=1)
    out["tot_abs"] = np.stack([np.abs(R).sum((1, 2)), (np.abs(R) * hi).sum((1, 2)), (np.abs(R) * lo).sum((1, 2)),
                               np.abs(A).sum((1, 2)), (Z * Z).sum((1, 2))], axis=1)
    tot = take("tot", tot)
    # k_coeff
    meanA = take("meanA", tot[:, 3].sum() / (LD(n) * P))
    out["ratio"] = np.sqrt(tot[:, 4].sum()) / LD(consts.normF)
    ratio = take("ratio", out["ratio"])
    cr = tot[:, 0] / P / meanA
    coeff = take("coeff", np.where(cr > 0, cr, LD(0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        b1c = take("b1c", (tot[:, 1] / tot[:, 5] - tot[:, 2] / tot[:, 6]) / meanA)
    B1, cbar, meanA1 = LD(state0["B1"]), LD(state0.get("cbar", 0.0)), LD(state0.get("meanA1", 0.0))
    Aoff, Mdark, skip = Aoff0, None, not get_darkfield
    out["dark_ran"] = False
    if get_darkfield:
        v = (f64(dev["coeff"]) if "coeff" in dev else coeff) < 1
        k = int(v.sum())
        skip = k == 0
        out["k"] = k
        if k:
            cv, bv = coeff[v], b1c[v]
            t1, t2, t3, t4 = (cv * cv).sum(), cv.sum(), bv.sum(), (cv * bv).sum()
            t5 = t2 * t3 - k * t4
            if "coeff" in dev:  # the kernel's own t5, sequential float64 sums in image order
                c64, b64 = f64(dev["coeff"])[v], f64(dev["b1c"])[v] if "b1c" in dev else f64(bv)
                s2 = s3 = s4 = f64(0)
                for c_, b_ in zip(c64, b64):
                    s2, s3, s4 = s2 + c_, s3 + b_, s4 + c_ * b_
                zero = (s2 * s3 - f64(k) * s4) == 0
            else:
                zero = t5 == 0
            out["t"] = (t1, t2, t3, t4, t5)
            b1 = LD(0) if zero else (t1 * t3 - t2 * t4) / t5
            out["b1_raw"] = b1
            b1 = max(b1, LD(0))
            cap = LD(consts.b_up) / meanF
            B1 = b1 if b1 < cap else cap
            cbar = t2 / k
            meanA1 = (tot[v, 0] / P).sum() / k - cbar * meanF
    B1, cbar, meanA1 = take("B1", B1), take("cbar", cbar), take("meanA1", meanA1)
    if get_darkfield and not skip:
        out["dark_ran"] = True
        boff = B1 * meanF - B1 * Fw
        X = ((R[v].sum(0) / k - cbar * Fw) - meanA1) - boff
        out["X"] = X
        out["X_abs"] = (np.abs(R[v]).sum(0) / k + np.abs(cbar * Fw) + abs(meanA1)) + np.abs(B1 * meanF) + np.abs(B1 * Fw)
        thr = LD(consts.lam_d) / (ENT2 * mu)
        Mdark = take("Mdark", shrink_ld(C @ X @ C.T, thr))
        Aoff = take("Aoff", shrink_ld(C.T @ Mdark @ C, thr) + boff)
    else:
        out["Aoff"] = Aoff
    out["skipdark"] = int(skip)
    mu1 = RHO * mu
    out["mu"] = mu1 if mu1 < LD(state0["mu_bar"]) else LD(state0["mu_bar"])
    out["mu_bar"] = state0["mu_bar"]
    out["iterations"] = int(state0["iterations"]) + 1
    # (ratio < tol is False for a NaN ratio, as on the device)
    out["done"] = int(bool(f64(ratio) < consts.tol) or out["iterations"] >= consts.max_iterations)
    return out


def next_state(out: dict) -> dict:
    """The state the next iteration starts from."""
    return {k: out[k] for k in ("What", "Fw", "Aoff", "coeff", "E", "Y", "B1", "cbar", "meanA1", "mu", "mu_bar",
                                "iterations")}


def fresh_state(c: Consts) -> dict:
    return state_dict(State(c))


def reweight(E, mxa, eps) -> np.ndarray:
    """k_weight / k_weight_scale: 1 / (|E / mXA| + eps) scaled to mean 1, float32."""
    E = np.asarray(E).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        wv = 1 / (np.abs(E / np.asarray(mxa).astype(LD)[None]) + LD(eps))
    return (wv * (LD(wv.size) / wv.sum())).astype(np.float32)


def linear_matrix_ld(src: int, dst: int) -> np.ndarray:
    """linear_matrix with the coordinate as lin_coord computes it (float64 scale and position), weights in longdouble."""
    m = np.zeros((dst, src), LD)
    scale = np.float64(src) / np.float64(dst)
    for i in range(dst):
        s = (i + 0.5) * scale - 0.5
        i0 = int(np.floor(s))
        f = LD(s) - i0
        if i0 < 0:
            i0, f = 0, LD(0)
        if i0 >= src - 1:
            i0, f = src - 1, LD(0)
        m[i, i0] += 1 - f
        m[i, min(i0 + 1, src - 1)] += f
    return m


def upsample_fields(flat_w, dark_w, ty, tx):
    """k_upsample: (ty, tx) float32 flat (divided by its mean) and dark from the float64 working-grid fields."""
    w = np.asarray(flat_w).shape[0]
    my, mx = linear_matrix_ld(w, ty), linear_matrix_ld(w, tx)
    flat = my @ np.asarray(flat_w).astype(LD) @ mx.T
    dark = my @ np.asarray(dark_w).astype(LD) @ mx.T
    return (flat / (flat.sum() / LD(ty * tx))).astype(np.float32), dark.astype(np.float32)


def apply_mirrored(tiles, flat, dark):
    """ShadeOp of mg_shadeop.h: v = (x - dark) / flat in float32 (float64 for float64 tiles), plain IEEE; integer
    outputs v > 0 ? v : 0, then v < max ? v : max, then truncated -- so NaN becomes 0 and +inf max."""
    tiles = np.asarray(tiles)
    wide = np.float64 if tiles.dtype == np.float64 else np.float32
    with np.errstate(all="ignore"):
        v = (tiles.astype(wide) - np.asarray(dark, np.float32).astype(wide)) / np.asarray(flat, np.float32).astype(wide)
    if tiles.dtype.kind != "u":
        return v.astype(tiles.dtype)
    top = wide(np.iinfo(tiles.dtype).max)
    v = np.where(v > 0, v, wide(0))
    v = np.where(v < top, v, top)
    return v.astype(np.uint32).astype(tiles.dtype)


def mirrored_fit_working(D, get_darkfield=True, max_iterations=500, optimization_tol=1e-6,
                         max_reweight_iterations=10, reweighting_tol=1e-2, epsilon=0.1, round32=True):
    """fit_working with the device's float32 roundings of E, Y and the weights: (flat, dark, iterations per pass,
    stop ratios of the last two iterations of every pass), the fields float64."""
    D = np.asarray(D, np.float32)
    c = Consts(D.astype(np.float64), get_darkfield, 1.0, 1.0, max_iterations, optimization_tol)
    weight = np.ones(D.shape, np.float32)
    flat_last, dark_last = np.ones(D.shape[1:]), np.zeros(D.shape[1:])
    iterations, ratios = [], []
    table = cos_table(c.w)
    flat = dark = None
    for _ in range(max_reweight_iterations):
        st, hist = fresh_state(c), []
        while True:
            o = alm_stages(st, D, weight, c, get_darkfield, round32=round32, table=table)
            hist.append(float(o["ratio"]))
            st = next_state(o)
            if o["done"]:
                break
        iterations.append(st["iterations"])
        ratios.append(hist[-2:])
        fw, coeff = np.asarray(st["Fw"]).astype(np.float64), np.asarray(st["coeff"]).astype(np.float64)
        a_off = np.asarray(st["Aoff"]).astype(np.float64) + float(st["B1"]) * fw
        mxa = (fw[None] * coeff[:, None, None] + a_off[None]).mean(0)
        weight = reweight(st["E"], mxa, epsilon)
        flat = mxa - a_off
        flat = flat / flat.mean()
        dark = a_off if get_darkfield else np.zeros_like(a_off)
        mad_f = np.abs(flat - flat_last).sum() / np.abs(flat_last).sum()
        dd = np.abs(dark - dark_last).sum()
        mad_d = 0.0 if dd < 1e-7 else dd / max(np.abs(dark_last).sum(), 1e-6)
        flat_last, dark_last = flat, dark
        if max(mad_f, mad_d) <= reweighting_tol:
            break
    return flat, dark, iterations, ratios


# ---- inputs shared by tests/test_cpu_shading.py (which checks their conditions with the oracle) and
# tests/test_gpu_shading_stages.py (which runs them on the device)

# name -> (tiles builder arguments, W, iterations k0 before the one under test)
STAGE_CASES = {
    "n8_w128_fresh": ("stack8", 128, 0),
    "n8_w128_k7": ("stack8", 128, 7),
    "n5_w33_k7": ("stack5", 33, 7),
    "n2_w50_fresh": ("stack2", 50, 0),
    "n2_w50_k1": ("stack2", 50, 1),
    "n300_w24_k3": ("gains300", 24, 3),
    "n8_w1_k2": ("stack8s", 1, 2),
}


def stage_tiles(kind: str) -> np.ndarray:
    """u16 training tiles of the staged cases (synthetic_stack needs about 64 pixels for its beads)."""
    if kind == "stack8":
        return synthetic_stack(n=8, size=256, seed=2)[0]
    if kind == "stack8s":
        return synthetic_stack(n=8, size=64, seed=2)[0]
    if kind == "stack5":
        return synthetic_stack(n=5, size=64, seed=3)[0]
    if kind == "stack2":
        return synthetic_stack(n=2, size=64, seed=STACK2_SEED)[0]
    if kind == "gains300":  # 300 tiles cut from 4 synthetic ones, each with a gain of its own
        base = synthetic_stack(n=4, size=64, seed=6)[0].astype(np.float64)
        gains = np.random.default_rng(6).uniform(0.4, 1.6, 300)
        return np.clip(np.rint(base[np.arange(300) % 4] * gains[:, None, None]), 0, 65535).astype(np.uint16)
    raise KeyError(kind)


STACK2_SEED = 1  # both coeff >= 1 after iteration 1 (1.011, 1.085), one below after iteration 2 (0.964, 1.036)


def run_oracle(D, k, get_darkfield=True):
    """(Consts, State after k oracle iterations, list of coeff after each) on the working stack D."""
    D = np.asarray(D, np.float64)
    c = Consts(D, get_darkfield)
    st, coeffs = State(c), []
    for _ in range(k):
        alm_step(st, D, np.ones_like(D), c)
        coeffs.append(st.coeff.copy())
    return c, st, coeffs


# three reweighting passes at most: enough to run a pass on reweighted data, and the mirrored oracle stays quick
FIT_CASES = {
    "t64x96_ws128": ("crop6", dict(working_size=128, max_reweight_iterations=3)),
    "t64x96_ws8": ("crop6", dict(working_size=8, max_reweight_iterations=3)),
    "t96_nodark": ("stack8m", dict(get_darkfield=False, max_reweight_iterations=3)),
}


def fit_tiles(kind: str) -> np.ndarray:
    if kind == "crop6":  # 6 tiles of 64 x 96: the same window of every 96 x 96 tile, so the fields stay common
        return np.ascontiguousarray(synthetic_stack(n=6, size=96, seed=12)[0][:, 16:80, :])
    if kind == "stack8m":
        return synthetic_stack(n=8, size=96, seed=8)[0]
    raise KeyError(kind)


_fit_cache = {}


def fit_three_ways(name: str, D=None):
    """(float64 oracle (flat, dark, its), mirrored oracle (flat, dark, its, last ratios)) of a FIT_CASES entry on its
    working stack (downsample_exact of its tiles unless D, the device's, is given); computed once per process."""
    if name not in _fit_cache:
        kind, kw = FIT_CASES[name]
        tiles = fit_tiles(kind)
        w = min(kw.get("working_size", 128), *tiles.shape[1:])
        if D is None:
            D = downsample_exact(tiles, w)
        kk = {k: v for k, v in kw.items() if k != "working_size"}
        _fit_cache[name] = (fit_working(D, **kk), mirrored_fit_working(D, **kk))
    return _fit_cache[name]
