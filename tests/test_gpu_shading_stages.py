"""Shading model on the MI355X, kernel by kernel (DESIGN.md §4 "shading", "GPU against the oracle"): every fit and
apply kernel of csrc/mg_shading.hip against the staged restatement of tests/ref_shading.py.  A chain of dependent
float kernels is compared stage by stage: each stage's reference is computed in np.longdouble from the DEVICE'S inputs
to that stage, with the float32 roundings of E and Y where the kernel has them, so every tolerance is a forward-error
bound of that stage's own arithmetic (u = 2^-53 per float64 rounding) and not the 1e-4 of a whole iteration.

Every test asserts the condition it was built for (a ragged chunk, n > 256, two workgroup columns, ...)."""
import numpy as np
import pytest
import torch

import ref_shading as rs
from oracle import ref_pipeline as rp

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0**-53

# workspace regions, scalar slots, flag words and the per-image totals (include/magnify_hip.h)
R_D, R_E, R_Y, R_WEIGHT, R_WHAT, R_FW, R_AOFF, R_M, R_T, R_COLMEAN, R_COLMIN, R_C, R_CT = range(13)
R_COEFF, R_TOT, R_PART, R_PARTF, R_GRAM, R_SC, R_FLAGS = range(13, 20)
(SC_MU, SC_MUBAR, SC_LF, SC_LD, SC_TOL, SC_NORMF, SC_BUP, SC_B1, SC_MEANF, SC_MEANA, SC_CBAR, SC_MEANA1,
 SC_RATIO) = range(13)
FL_DONE, FL_ITER, FL_MAXIT, FL_SKIPDARK = range(4)
TOT_R, TOT_RHI, TOT_RLO, TOT_A, TOT_Z2, TOT_NHI, TOT_NLO, TOT_B1C = range(8)
CHUNK, LANES = 1024, 256  # pixels per workgroup of k_update / k_weight; lanes of a workgroup


@pytest.fixture(scope="module")
def mg():
    import magnify_amd

    magnify_amd.hotpath.require_gpu()
    return magnify_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f64(x):
    return np.asarray(x).astype(np.float64)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def _report(what, err, bound):
    """Prints the largest error / bound of a stage (pytest -s shows it) and returns it."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    worst = float(np.max(q)) if q.size else 0.0
    print(f"{what}: max error / bound {worst:.3g}")
    return worst


def _cast(u16, dtype):
    if dtype == np.uint8:
        return (u16 >> 8).astype(np.uint8)
    if np.dtype(dtype).kind == "f":
        return (u16 + np.random.default_rng(9).random(u16.shape)).astype(dtype)  # not integers
    return u16.astype(dtype)


# ---- downsample ------------------------------------------------------------------------------------------------------

DOWN_SHAPES = [(8, 8, 8), (128, 128, 128), (129, 128, 128), (300, 211, 100), (257, 1031, 128), (8, 13, 1),
               (17, 40, 8)]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64])
@pytest.mark.parametrize("ty, tx, w", DOWN_SHAPES)
def test_downsample_is_exact(mg, dtype, ty, tx, w):
    rng = np.random.default_rng(ty * 7 + tx)
    tiles = _cast(rng.integers(0, 65536, size=(3, ty, tx)).astype(np.uint16), dtype)
    integer = np.dtype(dtype).kind == "u"
    if integer:
        tiles[2] = np.iinfo(dtype).max  # a saturated tile: its means are exactly the maximum
    got = mg.shading.working_stack(_dev(tiles), w).cpu().numpy()
    want = rs.downsample_exact(tiles, w)
    assert got.dtype == np.float32 and got.shape == (3, w, w)
    if integer:
        np.testing.assert_array_equal(got, want)
        assert (got[2] == np.iinfo(dtype).max).all()
    else:
        assert np.all(np.abs(got.astype(np.float64) - want) <= _ulp32(want))


@pytest.mark.parametrize("n, ty, tx, w", [(3, 7, 16, 8), (3, 16, 7, 8), (3, 16, 16, 0), (3, 200, 200, 129),
                                          (0, 16, 16, 8)])
def test_downsample_refusals_write_nothing(mg, n, ty, tx, w):
    tiles = torch.zeros((3, ty, tx), dtype=torch.uint16).cuda()
    out = torch.full((3 * 130 * 130,), -7.0, dtype=torch.float32).cuda()
    with pytest.raises(ValueError):
        mg.hotpath._call("mg_shading_downsample", tiles.data_ptr(), mg._native.MG_U16, n, ty, tx, w, out.data_ptr(),
                         mg.hotpath._stream())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- prepare: weight, per-pixel mean / min, Gram matrix, cosine table ---------------------------------------------


def _stack(n, w, seed=0):
    """(n, w, w) float32 working stack of positive intensities with a different level per image."""
    rng = np.random.default_rng(seed + 100 * n + w)
    return (rng.uniform(200, 3000, (n, 1, 1)) * (0.5 + rng.random((n, w, w)))).astype(np.float32)


def _read(f, region, dtype, shape):
    return f.view(region, dtype, shape).cpu().numpy()


@pytest.mark.parametrize("n, w", [(1, 1), (2, 8), (5, 33), (8, 128), (300, 24), (17, 128)])
def test_prepare(mg, n, w):
    d = _stack(n, w)
    f = mg.shading._Fitter(_dev(d))
    P = w * w
    dl = d.astype(LD)
    assert (_read(f, R_WEIGHT, torch.float32, (n, w, w)) == 1.0).all()
    np.testing.assert_array_equal(_read(f, R_COLMIN, torch.float64, (w, w)), d.min(0).astype(np.float64))
    # mean: n additions and one division, every partial sum at most sum|d|: n u sum|d| / n (the issue's bound; the
    # division's rounding is inside it because the first addition, to 0, is exact)
    mean = _read(f, R_COLMEAN, torch.float64, (w, w))
    worst = _report("colmean", np.abs(mean - dl.mean(0)), n * U * np.abs(dl).sum(0) / n)
    assert worst <= 1
    gram = _read(f, R_GRAM, torch.float64, (n, n))
    np.testing.assert_array_equal(gram, gram.T)
    flat = dl.reshape(n, P)
    # any summation order of P products: at most P roundings on a path, each at most u sum|d_a d_b|
    worst = _report("gram", np.abs(gram - flat @ flat.T), P * U * _f64(np.abs(flat) @ np.abs(flat).T))
    assert worst <= 1
    c, ct = _read(f, R_C, torch.float64, (w, w)), _read(f, R_CT, torch.float64, (w, w))
    np.testing.assert_array_equal(ct, c.T)
    worst = _report("table", np.abs(c - rs.cos_table(w)), rs.cos_table_bound(w))
    assert worst <= 1
    if (n, w) == (5, 33):
        assert P % LANES != 0  # a ragged last 256-lane group in k_gram's loop
    if n == 300:
        assert n > LANES
    if (n, w) == (17, 128):  # k_setup runs on a fixed grid: more values than it has lanes send it round again
        assert n * P > mg.hotpath.nat.DEFINES["MG_SHADING_SETUP_WALK"] * LANES


def test_begin_resets_a_stack_of_more_values_than_its_grid_has_lanes(mg):
    """k_begin runs on a fixed grid and strides over the n w^2 values of E and Y: 17 images at w = 128 send it round
    again ("Capped launches and who walks them twice").  The state of a fresh pass is exact: zeros and ones."""
    n, w = 17, 128
    assert n * w * w > mg.hotpath.nat.DEFINES["MG_SHADING_SETUP_WALK"] * LANES
    f = mg.shading._Fitter(_dev(_stack(n, w)))
    for region, dtype, shape in ((R_E, torch.float32, (n, w, w)), (R_Y, torch.float32, (n, w, w)),
                                 (R_WHAT, torch.float64, (w, w)), (R_FW, torch.float64, (w, w)),
                                 (R_AOFF, torch.float64, (w, w)), (R_COEFF, torch.float64, (n,))):
        f.view(region, dtype, shape).fill_(3.0)
    f.begin()
    for region in (R_E, R_Y):
        assert not _read(f, region, torch.float32, (n, w, w)).any()
    for region in (R_WHAT, R_FW, R_AOFF):
        assert not _read(f, region, torch.float64, (w, w)).any()
    assert (_read(f, R_COEFF, torch.float64, (n,)) == 1.0).all()
    flags = _read(f, R_FLAGS, torch.int32, (8,))
    assert flags[FL_DONE] == 0 and flags[FL_ITER] == 0
    assert (_read(f, R_WEIGHT, torch.float32, (n, w, w)) == 1.0).all()  # (k_setup's, untouched)


# ---- DCT -------------------------------------------------------------------------------------------------------------


def _dct_bound(left, x, right):
    """Two chained FMA dot products of W terms: each is within W u |l|.|r| of its exact value, and the second also
    carries the first's error: (2 W + W^2 u) u |L| |X| |R| <= 2.1 W u |L| |X| |R|."""
    w = x.shape[0]
    return 2.1 * w * U * _f64(np.abs(left).astype(LD) @ np.abs(x).astype(LD) @ np.abs(right).astype(LD))


@pytest.mark.parametrize("scale", [1.0, 1e6])
@pytest.mark.parametrize("w", [1, 2, 3, 8, 33, 100, 127, 128])
def test_dct_within_its_forward_bound(mg, w, scale):
    rng = np.random.default_rng(w)
    f = mg.shading._Fitter(_dev(_stack(2, w)))
    c = f.cos_table().astype(LD)
    true = rs.cos_table(w)
    cb = rs.cos_table_bound(w).astype(LD)
    x = scale * rng.standard_normal((w, w))
    xin, out = _dev(x), torch.empty((w, w), dtype=torch.float64).cuda()
    xl, ax = x.astype(LD), np.abs(x).astype(LD)
    if w == 8:
        from scipy.fft import dctn

        assert np.abs(_f64(true @ xl @ true.T) - dctn(x, norm="ortho")).max() <= 1e-13 * scale
    both = []
    for inverse, (lt, rt) in ((0, (c, c.T)), (1, (c.T, c))):
        f._call("mg_shading_dct2", xin.data_ptr(), out.data_ptr(), inverse)
        got = out.cpu().numpy()
        b_prod = _dct_bound(lt, x, rt)
        worst = _report(f"dct2 inverse={inverse} against the device's table", np.abs(got - lt @ xl @ rt), b_prod)
        assert worst <= 1
        tl, tr = (true, true.T) if not inverse else (true.T, true)
        bl, br = (cb, cb.T) if not inverse else (cb.T, cb)
        # the table's own error, once on each side: bound_C |X| |C^T| + |C| |X| bound_C^T
        b_true = b_prod + _f64(bl @ ax @ np.abs(tr) + np.abs(tl) @ ax @ br)
        worst = _report(f"dct2 inverse={inverse} against the true transform", np.abs(got - tl @ xl @ tr), b_true)
        assert worst <= 1
        both.append((got, b_true))
    # round trip: idct2(dct2(x)) = x within the forward transform's bound carried through |C^T| . |C| and the
    # inverse's own bound on the transformed data
    fwd, b_fwd = both[0]
    f._call("mg_shading_dct2", _dev(fwd).data_ptr(), out.data_ptr(), 1)
    back = out.cpu().numpy()
    ac = np.abs(true)
    b_back = (_f64(ac.T @ b_fwd.astype(LD) @ ac) + _dct_bound(c.T, fwd, c)
              + _f64(cb.T @ np.abs(fwd).astype(LD) @ ac + ac.T @ np.abs(fwd).astype(LD) @ cb))
    worst = _report("dct2 round trip", np.abs(back - x), b_back)
    assert worst <= 1


# ---- one ALM iteration, staged ---------------------------------------------------------------------------------------


def _snapshot(f):
    """Every region of the workspace the stages read or write, as host arrays."""
    n, w = f.n, f.w
    sc = _read(f, R_SC, torch.float64, (32,))
    fl = _read(f, R_FLAGS, torch.int32, (8,))
    return dict(E=_read(f, R_E, torch.float32, (n, w, w)), Y=_read(f, R_Y, torch.float32, (n, w, w)),
                What=_read(f, R_WHAT, torch.float64, (w, w)), Fw=_read(f, R_FW, torch.float64, (w, w)),
                Aoff=_read(f, R_AOFF, torch.float64, (w, w)), M=_read(f, R_M, torch.float64, (w, w)),
                coeff=_read(f, R_COEFF, torch.float64, (n,)), tot=_read(f, R_TOT, torch.float64, (n, 8)),
                sc=sc, fl=fl, mu=sc[SC_MU], mu_bar=sc[SC_MUBAR], B1=sc[SC_B1], cbar=sc[SC_CBAR],
                meanA1=sc[SC_MEANA1], meanF=sc[SC_MEANF], meanA=sc[SC_MEANA], ratio=sc[SC_RATIO],
                iterations=int(fl[FL_ITER]))


class _DeviceConsts:
    def __init__(self, f, sc):
        self.lam_f, self.lam_d, self.tol, self.normF, self.b_up = (sc[SC_LF], sc[SC_LD], sc[SC_TOL], sc[SC_NORMF],
                                                                   sc[SC_BUP])
        self.max_iterations = f.max_iterations


_runs = {}


def _stage_run(mg, name):
    """(fitter, D, snapshot, state after one iteration without darkfield, the same with) of a staged case; the
    device work is done once per case."""
    if name not in _runs:
        kind, w, k0 = rs.STAGE_CASES[name]
        tiles = rs.stage_tiles(kind)
        d = mg.shading.working_stack(_dev(tiles), w)
        f = mg.shading._Fitter(d)
        f.begin()
        f.iterate(k0)
        snap = f.ws.clone()  # the whole workspace: state, scalars and flags
        s0 = _snapshot(f)
        f._call("mg_shading_alm_iterate", 1, 0)
        plain = _snapshot(f)
        f.ws.copy_(snap)
        assert torch.equal(f.ws, snap)
        f._call("mg_shading_alm_iterate", 1, 1)
        dark = _snapshot(f)
        _runs[name] = (f, d.cpu().numpy(), s0, plain, dark)
    return _runs[name]


def _float32_stage(what, got, ref_ld, bound, near_threshold, failures):
    """A float32 store of a float64 value known within `bound` of ref_ld: the bits of float32(ref_ld), except where
    ref_ld lies within `bound` of a float32 rounding boundary (the float64 value may round to the neighbour) or of
    the shrink threshold (the float64 value may be on its other side, at most `bound` away): there 1 float32 ulp
    plus the bound.  Returns the share of excepted entries."""
    want = ref_ld.astype(np.float32)
    up = np.nextafter(want, np.float32(np.inf)).astype(LD)
    down = np.nextafter(want, np.float32(-np.inf)).astype(LD)
    wl = want.astype(LD)
    edge = np.minimum(np.abs(ref_ld - (wl + up) / 2), np.abs(ref_ld - (wl + down) / 2))
    # (an exact 0 -- shrunk away, and not near the threshold -- is 0 in float64 too: it has no rounding to differ in)
    excepted = ((edge <= bound) & (ref_ld != 0)) | near_threshold
    same = got.view(np.uint32) == want.view(np.uint32)
    same |= (got == 0) & (want == 0)  # (+0 and -0: shrink returns +0, a difference of equal values too)
    strict_ok = same | excepted
    loose = np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.maximum(_ulp32(want), _ulp32(got)) + bound
    share = float(excepted.mean())
    print(f"{what}: {int((~same).sum())} of {same.size} entries differ from the reference's float32 bits, "
          f"{int(excepted.sum())} in the 1-ulp exception")
    if not (strict_ok.all() and loose.all()):
        failures.append((what, int((~strict_ok).sum()), int((~loose).sum())))
    if share > 1e-3:
        failures.append((what + " exception share", share))
    return share


@pytest.mark.parametrize("name", list(rs.STAGE_CASES))
def test_alm_iteration_stage_by_stage(mg, name):
    kind, w, k0 = rs.STAGE_CASES[name]
    f, D, s0, a, b = _stage_run(mg, name)
    n, P = f.n, w * w
    nch, nbp = -(-P // CHUNK), -(-P // LANES)
    # the conditions the case was built for
    if name == "n5_w33_k7":
        assert P % CHUNK != 0 and nch == 2 and P % LANES != 0 and nbp == 5
    if name == "n300_w24_k3":
        assert n > LANES
    if name == "n8_w1_k2":
        assert P == 1
    assert s0["iterations"] == k0 and not s0["fl"][FL_DONE]
    if k0 == 0:
        assert not s0["Fw"].any() and not s0["E"].any() and (s0["coeff"] == 1).all()  # A = 0 in the first mean
    consts = _DeviceConsts(f, s0["sc"])
    table = _read(f, R_C, torch.float64, (w, w))
    weight = _read(f, R_WEIGHT, torch.float32, (n, w, w))
    failures = []

    def check(what, got, want, bound):
        worst = _report(f"{name} {what}", np.abs(np.asarray(got, np.float64).astype(LD) - want), bound)
        if not worst <= 1:
            failures.append((what, worst))

    def stages(run, get_dark):
        dev = {k: run[k] for k in ("What", "Fw", "E", "Y", "coeff", "meanF", "meanA", "ratio", "B1", "cbar", "meanA1")}
        dev["tot"] = run["tot"][:, :7]
        dev["b1c"] = run["tot"][:, TOT_B1C]
        if get_dark:
            dev["Mdark"] = run["M"]
            dev["Aoff"] = run["Aoff"]
        else:
            dev["M"] = run["M"]
        return rs.alm_stages(s0, D, weight, consts, get_dark, dev=dev, table=table)

    ref = stages(a, False)
    C = table.astype(LD)
    aC = np.abs(C)
    mu = LD(s0["mu"])
    Dl, E0, Y0 = D.astype(LD), s0["E"].astype(LD), s0["Y"].astype(LD)
    Fw0, Aoff0, c0 = s0["Fw"].astype(LD), s0["Aoff"].astype(LD), s0["coeff"].astype(LD)

    # M: per image a = fw c + ao (2 roundings), d - a, - e, y / mu, the sum of the two (5 on the longest path), n
    # accumulations, / n (/ ent1 = 1 is exact): (n + 6) u on the mean of the terms' magnitudes
    terms0 = np.abs(Fw0[None] * c0[:, None, None]) + np.abs(Aoff0)[None] + np.abs(Dl) + np.abs(E0) + np.abs(Y0 / mu)
    check("M", a["M"], ref["M"], (n + 6) * U * _f64(terms0.sum(0) / n))

    # W_hat = shrink(W_hat0 + C M C^T, lam_f / (ent1 mu)) from the device's M: the product's bound; the addition (1);
    # the threshold's division (ent1 mu is exact) and the subtraction (2 more, on |sum| + thr).  shrink is 1-Lipschitz.
    Ml = a["M"].astype(LD)
    prod = np.abs(C @ Ml @ C.T)
    thr_f = _f64(LD(consts.lam_f) / mu)
    check("W_hat", a["What"], ref["What"],
          _dct_bound(C, a["M"], C.T) + 3 * U * _f64(np.abs(s0["What"]) + prod + thr_f))

    # F_w = C^T W_hat C from the device's W_hat
    check("F_w", a["Fw"], ref["Fw"], _dct_bound(C.T, a["What"], C))

    # mean(F_w): 8 levels of the 256-lane tree, nbp sequential partial sums, one division
    check("mean F_w", a["meanF"], ref["meanF"], (8 + nbp + 1) * U * _f64(np.abs(a["Fw"]).sum() / P))

    # E = float32(shrink(e + (((d - a) - e) + y / mu) / ent1, weight / (ent1 mu))) from the device's F_w:
    # a (2), d - a, - e, y / mu and the sum, e + (6 on the longest path); the threshold (1), the subtraction (1)
    Fwl = a["Fw"].astype(LD)
    termsE = (np.abs(Fwl[None] * c0[:, None, None]) + np.abs(Aoff0)[None] + np.abs(Dl) + 2 * np.abs(E0)
              + np.abs(Y0 / mu))
    boundE = 8 * U * _f64(termsE + ref["E_thr"])
    near = np.abs(np.abs(ref["E_pre"]) - ref["E_thr"]) <= boundE
    _float32_stage(f"{name} E", a["E"], ref["E_ld"], boundE, near, failures)
    if k0 >= 7:
        assert (a["E"] > 0).any() and (a["E"] == 0).any()
    if name == "n5_w33_k7":
        assert (a["E"] < 0).any()  # all three branches of the shrink

    # Y = float32(y + mu ((d - a) - E)) from the device's E: a (2), d - a, - E, mu z, y + (6 on the longest path)
    El = a["E"].astype(LD)
    termsY = np.abs(Y0) + mu * (np.abs(Fwl[None] * c0[:, None, None]) + np.abs(Aoff0)[None] + np.abs(Dl) + np.abs(El))
    _float32_stage(f"{name} Y", a["Y"], ref["Y_ld"], 6 * U * _f64(termsY), np.zeros(D.shape, bool), failures)

    # per-image totals from the device's E and F_w: a lane adds at most 4 pixels, the tree has 8 levels, the chunks
    # are added in k_coeff (nch): 12 + nch accumulations, plus the roundings of the term itself -- r = d - E (1),
    # a (2), z = (d - a) - E (4, then z z: 2 |z| dz + u z^2)
    acc = 12 + nch
    tot = a["tot"]
    ta = ref["tot_abs"]
    for col, label, own in ((TOT_R, "R", 1), (TOT_RHI, "R hi", 1), (TOT_RLO, "R lo", 1), (TOT_A, "A", 2)):
        check(f"total {label}", tot[:, col], ref["tot"][:, col], (acc + own) * U * _f64(ta[:, col]))
    A1 = Fwl[None] * c0[:, None, None] + Aoff0[None]
    Zl = (Dl - A1) - El
    dz = 4 * U * (np.abs(Dl) + np.abs(Fwl[None] * c0[:, None, None]) + np.abs(Aoff0)[None] + np.abs(El))
    check("total Z^2", tot[:, TOT_Z2], ref["tot"][:, TOT_Z2],
          _f64((2 * np.abs(Zl) * dz).sum((1, 2)) + (acc + 1) * U * ta[:, TOT_Z2]))
    hi = a["Fw"] > a["meanF"] - rs.EPS_HI_LO
    lo = a["Fw"] < a["meanF"] + rs.EPS_HI_LO
    if not ((tot[:, TOT_NHI] == hi.sum()).all() and (tot[:, TOT_NLO] == lo.sum()).all()):
        failures.append(("counts hi / lo", tot[:, TOT_NHI].tolist(), int(hi.sum()), int(lo.sum())))
    print(f"{name}: {int(hi.sum())} hi and {int(lo.sum())} lo pixels of {P}")
    if P > 1 and k0 >= 2:  # (the first iterations keep only the constant term of W_hat: F_w is flat, every pixel both)
        assert 0 < hi.sum() < P and 0 < lo.sum() < P and hi.sum() != lo.sum()  # proper subsets: a swap would show

    # mean(A): n sequential additions, one division (n P is exact); ratio: n additions under the square root (which
    # halves the relative error), the root, the division
    check("mean A", a["meanA"], ref["meanA"], (n + 1) * U * _f64(np.abs(tot[:, TOT_A]).sum() / (n * P)))
    check("ratio", a["ratio"], ref["ratio"], (n / 2 + 2) * U * _f64(ref["ratio"]))
    # coeff = max(R / P / mean A, 0): two divisions
    check("coeff", a["coeff"], ref["coeff"], 2 * U * _f64(np.abs(ref["coeff"])))
    # B1c = (R hi / n hi - R lo / n lo) / mean A: two quotients, their difference (3 on the magnitudes), the division
    tl = tot.astype(LD)
    mag = (np.abs(tl[:, TOT_RHI] / tl[:, TOT_NHI]) + np.abs(tl[:, TOT_RLO] / tl[:, TOT_NLO])) / abs(LD(a["meanA"]))
    check("B1c", tot[:, TOT_B1C], ref["b1c"], 4 * U * _f64(mag))

    # scalars of the iteration: exact
    mu1 = min(_f64(1.5) * s0["mu"], s0["mu_bar"])
    for run in (a, b):
        if not (run["mu"] == mu1 and run["iterations"] == k0 + 1 and run["fl"][FL_DONE] == ref["done"] == 0
                and run["fl"][FL_MAXIT] == f.max_iterations):
            failures.append(("mu / iterations / done", run["mu"], mu1, run["fl"].tolist()))
    # without darkfield the darkfield state is left alone
    for key in ("Aoff", "B1", "cbar", "meanA1"):
        if not np.array_equal(a[key], s0[key]):
            failures.append((key + " changed by an iteration without darkfield",))
    if a["fl"][FL_SKIPDARK] != s0["fl"][FL_SKIPDARK]:
        failures.append(("skip-dark changed by an iteration without darkfield",))

    # the darkfield run: the step only feeds the next iteration, so everything before it has the same bits
    for key in ("What", "Fw", "E", "Y", "tot", "coeff", "meanF", "meanA", "ratio"):
        if not np.array_equal(a[key], b[key]):
            failures.append((key + " differs between the runs with and without darkfield",))
    refd = stages(b, True)
    below = b["coeff"] < 1
    k = int(below.sum())
    assert refd["k"] == k
    if b["fl"][FL_SKIPDARK] != int(k == 0) or refd["skipdark"] != int(k == 0):
        failures.append(("skip-dark", int(b["fl"][FL_SKIPDARK]), k))
    if name == "n2_w50_fresh":
        assert k == 0  # skipped: nothing of the darkfield state moves, and M still holds the mean
        for key in ("Aoff", "B1", "cbar", "meanA1"):
            if not np.array_equal(b[key], s0[key]):
                failures.append((key + " changed by a skipped darkfield step",))
        if not np.array_equal(b["M"], a["M"]):
            failures.append(("M changed by a skipped darkfield step",))
    elif name == "n2_w50_k1":
        assert s0["fl"][FL_SKIPDARK] == 1 and k == 1 and b["fl"][FL_SKIPDARK] == 0  # set, then cleared
    elif k0 > 0:
        assert 0 < (s0["coeff"] < 1).sum() < n and 0 < k < n
    if k > 0:
        assert refd["dark_ran"]
        t1, t2, t3, t4, t5 = (_f64(abs(t)) for t in refd["t"])
        b1 = _f64(abs(refd["b1_raw"]))
        cap = _f64(LD(consts.b_up) / abs(LD(b["meanF"])))
        # B1 with its cancellation (numerator and denominator are differences of products of sums), and the cap's
        # division; the clamps are 1-Lipschitz
        bB1 = U * cap if t5 == 0 else 8 * U * ((t1 * t3 + t2 * t4) / t5 + b1 * (t2 * t3 + k * t4) / t5) + U * cap
        check("B1", b["B1"], refd["B1"], bB1)
        # cbar = t2 / k: k - 1 additions of positive terms and the division
        check("cbar", b["cbar"], refd["cbar"], k * U * _f64(abs(refd["cbar"])))
        # mean(A1) = sum_V(R / P) / k - cbar mean F: per term a division and an accumulation (k + 1 on the path), / k,
        # the product, the difference
        magA1 = _f64(np.abs(tl[below, TOT_R] / P).sum() / k + abs(LD(b["cbar"]) * LD(b["meanF"])))
        check("mean A1", b["meanA1"], refd["meanA1"], (k + 4) * U * magA1)
        # the shrunk dark DCT (M after the darkfield step).  Its input X is overwritten in place, so the reference
        # forms X from the device's D, E, coeff, F_w and scalars; X's own roundings -- k accumulations of d - E (1),
        # / k, cbar fw and the difference, - mean A1, B1 mean F - B1 fw (on its own path), the last difference:
        # k + 6 on the longest path -- are pushed through |C| . |C^T| and added to the product's bound
        bX = (k + 6) * U * refd["X_abs"]
        thr_d = _f64(LD(consts.lam_d) / (rs.ENT2 * mu))
        prodX = np.abs(C @ refd["X"] @ C.T)
        check("dark DCT", b["M"], refd["Mdark"], _dct_bound(C, _f64(refd["X"]), C.T) + _f64(aC @ bX @ aC.T)
              + 3 * U * _f64(prodX + thr_d))
        # A_off = shrink(C^T M C, thr) + (B1 mean F - B1 fw) from the device's M: the product; threshold and
        # subtraction (3, as above); the two products, their difference and the sum (4)
        Md = b["M"].astype(LD)
        prodA = np.abs(C.T @ Md @ C)
        boff = abs(LD(b["B1"]) * LD(b["meanF"])) + np.abs(LD(b["B1"]) * Fwl)
        check("A_off", b["Aoff"], refd["Aoff"],
              _dct_bound(C.T, b["M"], C) + 4 * U * _f64(prodA + thr_d + boff))
        if name != "n8_w1_k2":
            assert np.abs(b["Aoff"]).max() > 0 and np.abs(b["M"]).max() > 0  # the shrinks left something to compare
    assert not failures, failures


# ---- gate and stop ---------------------------------------------------------------------------------------------------


def _fitter(mg, name, **kw):
    kind, w, _ = rs.STAGE_CASES[name]
    d = mg.shading.working_stack(_dev(rs.stage_tiles(kind)), w)
    return mg.shading._Fitter(d, **kw)


def test_done_gate_and_iteration_cap(mg):
    f1, f2 = _fitter(mg, "n5_w33_k7", max_iterations=3), _fitter(mg, "n5_w33_k7", max_iterations=3)
    for f, k in ((f1, 16), (f2, 3)):
        f.begin()
        f.iterate(k)
    assert torch.equal(f1.ws, f2.ws)  # the 13 gated iterations wrote nothing
    fl = _read(f1, R_FLAGS, torch.int32, (8,))
    assert fl[FL_DONE] == 1 and fl[FL_ITER] == 3 and fl[FL_MAXIT] == 3
    assert _read(f1, R_SC, torch.float64, (32,))[SC_RATIO] >= 1e-6  # stopped by the cap, not by the tolerance
    before = f1.ws.clone()
    f1.iterate(16)
    assert torch.equal(f1.ws, before)


def test_stop_by_tolerance(mg):
    f = _fitter(mg, "n5_w33_k7", optimization_tol=1.0)
    f.begin()
    f.iterate(16)
    fl = _read(f, R_FLAGS, torch.int32, (8,))
    sc = _read(f, R_SC, torch.float64, (32,))
    assert fl[FL_DONE] == 1 and fl[FL_ITER] == 1 and fl[FL_MAXIT] == 500
    assert sc[SC_RATIO] < 1.0 and sc[SC_TOL] == 1.0
    before = f.ws.clone()
    f.iterate(16)
    assert torch.equal(f.ws, before)


# ---- reweight --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["n5_w33_k7", "n8_w128_k7"])
def test_reweight(mg, name):
    f = _fitter(mg, name)
    n, w = f.n, f.w
    P = w * w
    f.run_pass()
    _, _, mxa = f.fields()
    E = _read(f, R_E, torch.float32, (n, w, w))
    assert (E != 0).any() and (E == 0).any()
    negative = mxa.copy()
    negative[::3, 1::2] *= -1.0
    if name == "n5_w33_k7":
        assert P % CHUNK != 0  # a ragged last chunk in k_weight
    for m in (mxa, negative):
        f.reweight(m, 0.1)
        got = _read(f, R_WEIGHT, torch.float32, (n, w, w))
        want = rs.reweight(E, m, 0.1)
        assert np.all(np.abs(got.astype(np.float64) - want) <= _ulp32(want))
        # every weight is within 2^-24 of its float64 value, whose mean is 1 up to float64 rounding
        assert abs(got.astype(np.float64).mean() - 1) <= 2.0**-24 * np.abs(got).astype(np.float64).mean() + 1e-12
        assert abs(got.astype(np.float64).mean() - 1) <= n * P * 2.0**-24
        np.testing.assert_array_equal(_read(f, R_E, torch.float32, (n, w, w)), E)


# ---- upsample --------------------------------------------------------------------------------------------------------


def _smooth(w, seed, level, amplitude):
    yy, xx = np.mgrid[0:w, 0:w] / max(w, 1)
    rng = np.random.default_rng(seed)
    a, b, c = rng.uniform(0.5, 2.0, 3)
    return level + amplitude * (np.sin(a * yy + b * xx) * np.cos(c * xx - yy) + 0.01 * rng.standard_normal((w, w)))


@pytest.mark.parametrize("w, ty, tx", [(8, 8, 8), (128, 128, 128), (8, 37, 301), (100, 300, 211), (128, 520, 1030),
                                       (1, 9, 9)])
def test_upsample(mg, w, ty, tx):
    launched = 256 * 256  # lanes of one k_upsample launch
    if (w, ty, tx) == (8, 37, 301):
        assert ty != tx and ty * tx < launched  # idle workgroups still have to write their partial sums
    if (w, ty, tx) == (128, 520, 1030):
        assert ty * tx > launched  # more than one trip of the grid-stride loop
    for seed, dark_level in ((w, 150.0), (w + 1, -40.0)):
        flat_w = _smooth(w, seed, 1.0, 0.3)
        dark_w = _smooth(w, seed + 7, dark_level, 60.0)
        flat, dark = mg.shading.full_fields(flat_w, dark_w, ty, tx, "cuda")
        flat, dark = flat.cpu().numpy(), dark.cpu().numpy()
        want_f, want_d = rs.upsample_fields(flat_w, dark_w, ty, tx)
        assert flat.shape == dark.shape == (ty, tx)
        assert np.all(np.abs(flat.astype(np.float64) - want_f) <= _ulp32(want_f))
        assert np.all(np.abs(dark.astype(np.float64) - want_d) <= _ulp32(want_d))
        mean = flat.astype(np.float64).mean()
        assert abs(mean - 1) <= 2.0**-24 * np.abs(flat).astype(np.float64).mean() + 1e-12
        assert abs(mean - 1) <= ty * tx * 2.0**-24
        if dark_level < 0:
            assert (dark < 0).any()
        if w == ty == tx:  # identity: the flat is only divided by its mean
            assert np.all(np.abs(flat - (flat_w / flat_w.mean())) <= _ulp32(want_f))
            np.testing.assert_array_equal(dark, dark_w.astype(np.float32))


# ---- apply fused with the stitch crop --------------------------------------------------------------------------------

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]


def _tiles(rng, shape, dtype):
    top = 255 if dtype == np.uint8 else 65535
    t = rng.integers(0, top + 1, size=shape)
    if np.dtype(dtype).kind == "f":
        return (t + rng.random(shape)).astype(dtype)
    return t.astype(dtype)


def _fields(rng, c, ty, tx, top):
    flats = (0.4 + 1.2 * rng.random((c, ty, tx))).astype(np.float32)
    darks = (0.3 * top * rng.random((c, ty, tx))).astype(np.float32)
    return flats, darks


def _check_apply(mg, tiles, flats, darks, overlap):
    c, t = tiles.shape[:2]
    corrected = np.stack([rs.apply_mirrored(tiles[i], flats[i], darks[i]) for i in range(c)])
    want = rp.stitch(corrected, overlap)
    dt, df, dd = _dev(tiles), _dev(flats), _dev(darks)
    got, minmax = mg.shading.apply_stitch(dt, overlap, df, dd)
    plain, none = mg.shading.apply_stitch(dt, overlap, df, dd, want_minmax=False)
    got, minmax = got.cpu().numpy(), minmax.cpu().numpy()
    assert none is None and got.dtype == tiles.dtype
    np.testing.assert_array_equal(got, want)  # (NaN equals NaN here: compared by position)
    assert got.tobytes() == plain.cpu().numpy().tobytes()
    planes = got.reshape(c * t, -1)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(minmax, np.stack([planes.min(1), planes.max(1)], 1).astype(np.float64))
    return got, corrected


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("overlap", [0, 1, 6, 18])
def test_apply_non_square_tiles_and_grid(mg, dtype, overlap):
    rng = np.random.default_rng(overlap)
    c, t, nr, nc, ty, tx = 2, 3, 2, 3, 19, 37
    tiles = _tiles(rng, (c, t, nr, nc, ty, tx), dtype)
    flats, darks = _fields(rng, c, ty, tx, 255 if dtype == np.uint8 else 65535)
    assert ty != tx and nr != nc and not np.array_equal(flats[0], flats[1])
    _, hy, hx = mg.hotpath.stitch_geometry(ty, tx, overlap)
    if overlap != 1:
        assert (nc * hx) % 4 != 0  # the last lane of a row writes fewer than 4 pixels (1, 3 and 1 of them)
    if overlap == 1:
        assert hy == ty - 1  # an odd clip: the far side loses the pixel
    got, corrected = _check_apply(mg, tiles, flats, darks, overlap)
    if np.dtype(dtype).kind == "u":
        assert (got == 0).any() and (got == np.iinfo(dtype).max).any()
    if overlap == 0:
        model = mg.shading.Shading(_dev(flats[1]), _dev(darks[1]))
        np.testing.assert_array_equal(model.apply(tiles[1]).cpu().numpy(), corrected[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_two_workgroup_columns(mg, dtype):
    rng = np.random.default_rng(11)
    ty, tx = 9, 1100
    gx = -(-tx // (256 * 4))
    assert gx > 1
    tiles = _tiles(rng, (1, 2, 1, 1, ty, tx), dtype)
    flats, darks = _fields(rng, 1, ty, tx, 255 if dtype == np.uint8 else 65535)
    _check_apply(mg, tiles, flats, darks, 0)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_apply_row_groups_walked_by_the_loop(mg, dtype):
    rng = np.random.default_rng(12)
    c, t, ty, tx = 3, 700, 20, 12
    planes, groups = c * t, -(-ty // 8)
    assert planes > 2048 and 2048 // planes == 0 and groups == 3  # gridDim.y = 1: one workgroup walks 3 row groups
    tiles = _tiles(rng, (c, t, 1, 1, ty, tx), dtype)
    flats, darks = _fields(rng, c, ty, tx, 65535)
    _check_apply(mg, tiles, flats, darks, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_special_values(mg, dtype):
    rng = np.random.default_rng(13)
    ty, tx = 16, 24
    top = 255 if dtype == np.uint8 else 65535
    tiles = _tiles(rng, (1, 1, 2, 2, ty, tx), dtype)
    flats, darks = _fields(rng, 1, ty, tx, top)
    tiles[..., 0, :] = 5
    darks[0, 0, :] = 9.0               # dark above the pixel -> 0
    flats[0, 1, :] = 1e-30             # a tiny flat -> max (inf for float tiles)
    tiles[..., 1, :] = 7
    darks[0, 1, :] = 0.0
    flats[0, 2, :] = -1.0              # a negative flat
    flats[0, 3, :] = 0.0               # 0 / 0 ...
    tiles[..., 3, :] = 7
    darks[0, 3, :] = 7.0
    flats[0, 4, :] = 0.0               # ... and x / 0 with x != dark, of either sign
    tiles[..., 4, :] = 7
    darks[0, 4, :12] = 1.0
    darks[0, 4, 12:] = 50.0
    tiles[..., 5, :] = top             # the largest pixel over a flat below 1
    flats[0, 5, :] = 0.5
    darks[0, 5, :] = 0.0
    if np.dtype(dtype).kind == "f":
        tiles[..., 6, 0:8] = np.nan
        tiles[..., 6, 8:16] = np.inf
        tiles[..., 6, 16:24] = -np.inf
    got, _ = _check_apply(mg, tiles, flats, darks, 0)
    rows = got[0, 0, :ty]
    if np.dtype(dtype).kind == "u":
        assert (rows[0] == 0).all() and (rows[1] == top).all() and (rows[3] == 0).all() and (rows[5] == top).all()
        assert (rows[4, :12] == top).all() and (rows[4, 12:tx] == 0).all()
    else:
        assert np.isnan(rows[3, :tx]).all() and np.isnan(rows[6, 0:8]).all() and (rows[6, 16:24] == -np.inf).all()
        assert (rows[4, :12] == np.inf).all() and (rows[4, 12:tx] == -np.inf).all()


def test_apply_refusals(mg):
    tiles = torch.zeros((1, 1, 1, 1, 8, 12), dtype=torch.uint16).cuda()
    fields = torch.ones((1, 8, 12), dtype=torch.float32).cuda()
    with pytest.raises(ValueError):
        mg.shading.apply_stitch(tiles, 8, fields, fields)  # overlap = ty
    many = torch.zeros((1, 65536, 1, 1, 1, 1), dtype=torch.uint8).cuda()
    one = torch.ones((1, 1, 1), dtype=torch.float32).cuda()
    with pytest.raises(ValueError):
        mg.shading.apply_stitch(many, 0, one, one)


# ---- the whole fit at shapes it has never had ------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(rs.FIT_CASES))
def test_fit_three_ways(mg, name):
    """The float64 oracle, the mirrored oracle (E, Y and the weights rounded to float32 as on the device) and the
    GPU on the same working stack.  The two oracles' difference is the size of the documented float32 deviation;
    the GPU may differ from the float64 oracle by 4 times that (summation order), with a floor."""
    kind, kw = rs.FIT_CASES[name]
    tiles = rs.fit_tiles(kind)
    n, ty, tx = tiles.shape
    w = min(kw.get("working_size", 128), ty, tx)
    if kind == "crop6":
        assert ty != tx and w == min(kw["working_size"], 64)
    np.testing.assert_array_equal(mg.shading.working_stack(_dev(tiles), w).cpu().numpy(), rs.downsample_exact(tiles, w))
    (flat, dark, its), (mflat, mdark, mits, _) = rs.fit_three_ways(name)
    model = mg.shading.fit(tiles, **kw)
    assert model.iterations == mits, (model.iterations, mits, its)
    f64 = rs.full_fields(flat, dark, ty, tx)
    mir = rs.full_fields(mflat, mdark, ty, tx)
    dev_flat, dev_dark = np.abs(_f64(f64[0]) - mir[0]).max(), np.abs(_f64(f64[1]) - mir[1]).max()
    tol_flat, tol_dark = max(4 * dev_flat, 1e-6), max(4 * dev_dark, 1e-6 * tiles.mean())
    err_flat = np.abs(model.flatfield.cpu().numpy().astype(np.float64) - f64[0]).max()
    err_dark = np.abs(model.darkfield.cpu().numpy().astype(np.float64) - f64[1]).max()
    print(f"{name}: flat |gpu - f64| {err_flat:.3g}, |mirrored - f64| {dev_flat:.3g}, tolerance {tol_flat:.3g}; "
          f"dark {err_dark:.3g}, {dev_dark:.3g}, {tol_dark:.3g}")
    assert err_flat <= tol_flat and err_dark <= tol_dark
    if not kw.get("get_darkfield", True):
        assert not model.darkfield.any() and np.abs(f64[0] - 1).max() > 0.05  # the flat itself was compared


def test_fit_of_equal_tiles(mg):
    model = mg.shading.fit(np.full((4, 64, 64), 1000, np.uint16))
    flat, dark = model.flatfield.cpu().numpy(), model.darkfield.cpu().numpy()
    assert np.isfinite(flat).all() and np.isfinite(dark).all()
    assert np.abs(flat - 1).max() <= 1e-6  # (the dark's constant part hangs on a tie at coeff = 1: not asserted)


def test_fit_of_zero_tiles_ends_and_raises(mg):
    tiles = np.zeros((3, 64, 64), np.uint16)
    with np.errstate(all="ignore"):
        f = mg.shading._Fitter(mg.shading.working_stack(_dev(tiles), 64), max_iterations=20)
        assert f.run_pass() == 20  # mu is infinite and the stop ratio 0 / 0: no stop test can hold, the cap ends the pass
        sc = _read(f, R_SC, torch.float64, (32,))
        assert np.isnan(sc[SC_RATIO]) and np.isnan(sc[SC_LF]) and np.isnan(f.fields()[0]).all()
        with pytest.raises(ValueError):
            mg.shading.fit(tiles, max_iterations=20)
