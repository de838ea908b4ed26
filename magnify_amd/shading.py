"""Shading correction without measured flat / dark images: a BaSiC fit (Peng et al., Nat. Commun. 8:14836, 2017)
of a flat- and a dark-field from the tiles themselves, and its apply -- the capability of the reference's
``basic_correct`` (preprocess.py:91-115, third-party basicpy there), built here on the HIP kernels of
``csrc/mg_shading.hip``.  The model and its constants are DESIGN.md §4 "shading".

    model = shading.fit(tiles)              # (N, ty, tx) training tiles, host array or device tensor
    corrected = model.apply(tiles)          # (x - dark) / flat, in the tiles' dtype
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _native as nat
from . import hotpath

# ALM iterations enqueued per host check of the device `done` word
BLOCK_ITERATIONS = 16

# workspace regions (include/magnify_hip.h, mg_shading_offset)
_D, _E, _Y, _WEIGHT, _WHAT, _FW, _AOFF, _M = 0, 1, 2, 3, 4, 5, 6, 7
_COLMEAN, _COLMIN, _COEFF, _GRAM, _SC, _FLAGS = 9, 10, 13, 17, 18, 19
_SC_B1 = 7


@dataclass
class Shading:
    """A fitted shading model: (ty, tx) float32 device fields and the ALM iterations of each reweighting pass."""

    flatfield: torch.Tensor
    darkfield: torch.Tensor
    iterations: list = field(default_factory=list)

    def apply(self, tiles, out=None):
        """(x - dark) / flat for tiles (..., ty, tx), in their dtype (integer outputs clamped to [0, max] and
        truncated); a device tensor of the same shape."""
        from .preprocess import to_device

        t = to_device(tiles)
        ty, tx = self.flatfield.shape
        if t.ndim < 2 or tuple(t.shape[-2:]) != (ty, tx):
            raise ValueError(f"tiles of shape {tuple(t.shape)} do not end in the fields' shape {(ty, tx)}")
        planes = t.numel() // (ty * tx)
        if out is None:
            out = torch.empty_like(t)
        elif not (out.is_contiguous() and out.shape == t.shape and out.dtype == t.dtype and out.device == t.device):
            raise ValueError("out must be a contiguous device tensor of the tiles' shape and dtype")
        if planes:
            apply_stitch(t.reshape(1, planes, 1, 1, ty, tx), 0, self.flatfield[None], self.darkfield[None],
                         want_minmax=False, out=out.view(1, planes, ty, tx))
        return out


def apply_stitch(tiles: torch.Tensor, overlap: int, flats: torch.Tensor, darks: torch.Tensor, want_minmax=True,
                 out: torch.Tensor | None = None, blend=None, shifts=None):
    """tiles (C, T, R, Cc, ty, tx) -> image (C, T, R*hy, Cc*hx) with (x - dark[c]) / flat[c] applied, and the
    per-plane min / max (C*T, 2) -- one launch for all channels (flats, darks: (C, ty, tx) float32).
    ``blend="linear"``: the seams blended as in ``hotpath.flatfield_stitch`` (mg_shading_apply_stitch_blend).
    ``shifts``: per-tile shifts as in ``hotpath.flatfield_stitch`` (mg_shading_apply_stitch_shift)."""
    hotpath.check_blend(blend)
    hotpath.require_gpu()
    c, t, nr, nc, ty, tx = tiles.shape
    if overlap < 0 or overlap >= ty or overlap >= tx:
        raise ValueError(f"Overlap ({overlap}) must be non-negative and smaller than tile size ({ty}x{tx}).")
    hotpath.check_blend(blend, overlap, ty, tx)
    if tuple(flats.shape) != (c, ty, tx) or tuple(darks.shape) != (c, ty, tx):
        raise ValueError("one (ty, tx) flat and dark field per channel")
    tiles = tiles.contiguous()
    flats = flats.to(tiles.device, torch.float32).contiguous()
    darks = darks.to(tiles.device, torch.float32).contiguous()
    _, hy, hx = hotpath.stitch_geometry(ty, tx, overlap)
    image = out if out is not None else torch.empty((c, t, nr * hy, nc * hx), dtype=tiles.dtype, device=tiles.device)
    minmax = None
    if want_minmax:
        minmax = hotpath._minmax_init(c * t, tiles.device).clone()
    if shifts is not None:
        table = hotpath.shift_tables(shifts, t, nr, nc, overlap, tiles.device)
        hotpath._call("mg_shading_apply_stitch_shift", tiles.data_ptr(), nat.dtype_code(tiles.dtype), c, t, nr, nc, ty, tx,
                      overlap, flats.data_ptr(), darks.data_ptr(), image.data_ptr(), hotpath._ptr(minmax),
                      table.data_ptr(), table.shape[0], t, int(blend is not None), hotpath._stream())
        return image, minmax
    hotpath._call("mg_shading_apply_stitch" if blend is None else "mg_shading_apply_stitch_blend", tiles.data_ptr(),
                  nat.dtype_code(tiles.dtype), c, t, nr, nc, ty, tx, overlap, flats.data_ptr(), darks.data_ptr(), image.data_ptr(), hotpath._ptr(minmax),
                  hotpath._stream())
    return image, minmax


class LazyShading:
    """A fitted shading correction pending on the tile stack (C, T, R, Cc, ty, tx), one field pair per channel.
    ``stitch`` fuses it with the crop/concat; any other access materialises it (overlap 0 per tile)."""

    def __init__(self, tiles: torch.Tensor, flats: torch.Tensor, darks: torch.Tensor):
        self.tiles, self.flatfield, self.darkfield = tiles, flats, darks
        self.shape, self.dtype = tuple(tiles.shape), tiles.dtype

    def materialize(self):
        c, t, nr, nc, ty, tx = self.shape
        out, _ = apply_stitch(self.tiles.reshape(c, t * nr * nc, 1, 1, ty, tx), 0, self.flatfield, self.darkfield,
                              want_minmax=False)
        return out.reshape(self.shape)


class _Fitter:
    """The device state of one fit: the working stack D, the ALM state and the constants of §4 "shading"."""

    def __init__(self, d: torch.Tensor, get_darkfield=True, smoothness_flatfield=1.0, smoothness_darkfield=1.0,
                 max_iterations=500, optimization_tol=1e-6):
        n, w = d.shape[0], d.shape[1]
        self.n, self.w, self.get_darkfield = n, w, bool(get_darkfield)
        self.max_iterations, self.tol = int(max_iterations), float(optimization_tol)
        lib = nat.lib()
        size = lib.mg_shading_workspace_bytes(n, w)
        if size < 0:
            raise ValueError(f"no shading workspace for {n} images of {w} x {w}")
        self.ws = torch.zeros(int(size), dtype=torch.uint8, device=d.device)
        self.view(_D, torch.float32, (n, w, w)).copy_(d)
        self._call("mg_shading_prepare")
        colmean = self.view(_COLMEAN, torch.float64, (w, w)).cpu().numpy()
        b_up = float(self.view(_COLMIN, torch.float64, (w * w,)).min().item())
        gram = self.view(_GRAM, torch.float64, (n, n)).cpu().numpy()
        m = colmean / colmean.mean()
        c = self.cos_table()
        s = float(np.abs(c @ m @ c.T).sum())
        self.lam_f = 0.5 * float(smoothness_flatfield) * s / 400
        self.lam_d = 0.2 * float(smoothness_darkfield) * s / 400
        self.norm2 = math.sqrt(max(float(np.linalg.eigvalsh(gram).max()), 0.0))
        self.norm_f = math.sqrt(max(float(np.trace(gram)), 0.0))
        self.b_up = b_up

    def view(self, region, dtype, shape):
        off = nat.lib().mg_shading_offset(self.n, self.w, region)
        count = int(np.prod(shape))
        nbytes = count * torch.empty((), dtype=dtype).element_size()
        return self.ws[off : off + nbytes].view(dtype).view(shape)

    def cos_table(self):
        return self.view(11, torch.float64, (self.w, self.w)).cpu().numpy()

    def _call(self, name, *args):
        hotpath._call(name, self.ws.data_ptr(), self.n, self.w, *args, hotpath._stream())

    def begin(self):
        mu = 12.5 / self.norm2 if self.norm2 > 0 else math.inf
        self._call("mg_shading_alm_begin", int(self.get_darkfield), self.max_iterations, mu, self.lam_f, self.lam_d,
                   self.tol, self.norm_f, self.b_up)

    def iterate(self, k):
        self._call("mg_shading_alm_iterate", int(k), int(self.get_darkfield))

    def flags(self):
        f = self.view(_FLAGS, torch.int32, (8,)).cpu()
        return bool(f[0]), int(f[1])

    def run_pass(self):
        self.begin()
        for _ in range(self.max_iterations // BLOCK_ITERATIONS + 1):
            self.iterate(BLOCK_ITERATIONS)
            done, it = self.flags()
            if done:
                return it
        raise RuntimeError("shading fit: the ALM pass did not report its end")

    def fields(self):
        """(flat, dark, mean_n XA) on the working grid at the end of a pass, float64 host arrays."""
        w = self.w
        fw = self.view(_FW, torch.float64, (w, w)).cpu().numpy()
        a_off = self.view(_AOFF, torch.float64, (w, w)).cpu().numpy()
        coeff = self.view(_COEFF, torch.float64, (self.n,)).cpu().numpy()
        b1 = float(self.view(_SC, torch.float64, (32,))[_SC_B1].item())
        a_off = a_off + b1 * fw
        mxa = (fw[None] * coeff[:, None, None] + a_off[None]).mean(0)
        flat = mxa - a_off
        flat = flat / flat.mean()
        dark = a_off if self.get_darkfield else np.zeros_like(a_off)
        return flat, dark, mxa

    def reweight(self, mxa, epsilon):
        self.view(_M, torch.float64, (self.w, self.w)).copy_(torch.from_numpy(np.ascontiguousarray(mxa)))
        self._call("mg_shading_reweight", float(epsilon))


def working_stack(tiles: torch.Tensor, w: int) -> torch.Tensor:
    """(N, ty, tx) device tiles -> (N, w, w) float32 area means (one launch)."""
    n, ty, tx = tiles.shape
    d = torch.empty((n, w, w), dtype=torch.float32, device=tiles.device)
    hotpath._call("mg_shading_downsample", tiles.data_ptr(), nat.dtype_code(tiles.dtype), n, ty, tx, w, d.data_ptr(),
                  hotpath._stream())
    return d


def full_fields(flat_w: np.ndarray, dark_w: np.ndarray, ty: int, tx: int, device):
    """Working-grid float64 fields -> (ty, tx) float32 device fields, the flat divided by its mean."""
    fw = torch.from_numpy(np.ascontiguousarray(flat_w, np.float64)).to(device)
    dw = torch.from_numpy(np.ascontiguousarray(dark_w, np.float64)).to(device)
    partial = torch.empty(256, dtype=torch.float64, device=device)
    flat = torch.empty((ty, tx), dtype=torch.float32, device=device)
    dark = torch.empty((ty, tx), dtype=torch.float32, device=device)
    hotpath._call("mg_shading_upsample", fw.data_ptr(), dw.data_ptr(), flat_w.shape[0], ty, tx, partial.data_ptr(),
                  flat.data_ptr(), dark.data_ptr(), hotpath._stream())
    return flat, dark


def _training_tiles(tiles, working_size):
    """Checks of fit()'s arguments (before any device work), then the (N, ty, tx) device tiles."""
    from .preprocess import SUPPORTED, to_device

    if not 8 <= int(working_size) <= 128:
        raise ValueError(f"working_size must be in [8, 128], got {working_size}")
    if isinstance(tiles, torch.Tensor):
        ok = str(tiles.dtype).replace("torch.", "") in SUPPORTED
    else:
        tiles = np.asarray(tiles)
        ok = tiles.dtype.name in SUPPORTED or tiles.dtype.kind in "iub"  # (to_device widens other integers)
    if not ok:
        raise ValueError(f"unsupported image dtype {tiles.dtype}")
    shape = tuple(tiles.shape)
    if len(shape) < 2:
        raise ValueError("tiles need at least two dimensions (..., ty, tx)")
    n, ty, tx = int(np.prod(shape[:-2])), shape[-2], shape[-1]
    if n < 2:
        raise ValueError(f"the fit needs at least 2 training tiles, got {n}")
    if ty < 8 or tx < 8:
        raise ValueError(f"tiles of {ty} x {tx}: at least 8 pixels on a side")
    return to_device(tiles).reshape(n, ty, tx)


def fit(tiles, *, get_darkfield=True, smoothness_flatfield=1.0, smoothness_darkfield=1.0, working_size=128,
        max_iterations=500, optimization_tol=1e-6, max_reweight_iterations=10, reweighting_tol=1e-2,
        epsilon=0.1) -> Shading:
    """Fit a BaSiC flat- and dark-field to training tiles (N, ty, tx) -- or any leading shape that flattens to N."""
    t = _training_tiles(tiles, working_size)
    n, ty, tx = t.shape
    w = min(int(working_size), ty, tx)
    fitter = _Fitter(working_stack(t, w), get_darkfield, smoothness_flatfield, smoothness_darkfield, max_iterations,
                     optimization_tol)
    flat_last, dark_last = np.ones((w, w)), np.zeros((w, w))
    iterations = []
    flat = dark = None
    for _ in range(int(max_reweight_iterations)):
        iterations.append(fitter.run_pass())
        flat, dark, mxa = fitter.fields()
        fitter.reweight(mxa, epsilon)
        mad_f = np.abs(flat - flat_last).sum() / np.abs(flat_last).sum()
        dd = np.abs(dark - dark_last).sum()
        mad_d = 0.0 if dd < 1e-7 else dd / max(np.abs(dark_last).sum(), 1e-6)
        flat_last, dark_last = flat, dark
        if max(mad_f, mad_d) <= reweighting_tol:
            break
    if flat is None:
        flat, dark = flat_last, dark_last
    flat_t, dark_t = full_fields(flat, dark, ty, tx, t.device)
    bad = int((~(torch.isfinite(flat_t) & (flat_t > 0))).sum().item())
    if bad:
        raise ValueError(f"the fitted flatfield has {bad} values that are not finite and positive")
    return Shading(flat_t, dark_t, iterations)
