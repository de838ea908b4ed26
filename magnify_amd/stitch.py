"""Stitcher (reference: src/magnify/stitch.py:7-50): crop ``overlap // 2`` (+ the odd remainder on
the far side) from every tile edge and butt the tiles together; no blending.  One HIP kernel does
the crop/concat, fused with a pending flat-field correction and with the per-plane min/max that
``to_uint8`` needs later.  ``blend="linear"`` (not in the reference) writes the same image with the overlap bands
around the inner seams mixed linearly from the tiles that cover them, in the same single pass.
``register="ncc"`` (not in the reference either) first measures where every tile really sits -- the displacement of
each pair of neighbours from the cross-correlation of their overlap strips, one integer shift per tile solved from
them (register.py) -- and stitches the tiles moved by these shifts."""
from __future__ import annotations

import numpy as np

from . import hotpath, preprocess, registry, shading
from . import register as registration
from .xr_lite import DataArray


class Stitcher:
    def __init__(self, overlap: int = 102, blend=None, register=None, max_shift: int = 8, register_channel=None,
                 register_time=0, min_score: float = 0.5):
        """``register="ncc"``: register the tiles before stitching them.  ``max_shift`` bounds the RELATIVE
        displacement of two neighbouring tiles (the search window of a seam, ``1 <= max_shift <= overlap // 4`` and
        at most 32, what the kernel's LDS tile takes),
        not a tile's absolute position error; a tile is moved by at most ``overlap // 2``.  ``register_channel``
        (name or index, None: the first) and ``register_time`` (an index: one shift table for every plane; "each":
        one per timepoint) select the planes that are correlated; a seam counts when its best score reaches
        ``min_score``."""
        if overlap < 0:
            raise ValueError("Overlap must be non-negative.")
        self.overlap = overlap
        self.blend = hotpath.check_blend(blend)
        self.register = registration.check_register(register, max_shift, overlap if register is not None else None)
        self.max_shift = int(max_shift)
        if isinstance(register_time, str):
            if register_time != "each":
                raise ValueError(f'register_time must be a time index or "each", got {register_time!r}')
        elif isinstance(register_time, bool) or int(register_time) != register_time:
            raise ValueError(f'register_time must be a time index or "each", got {register_time!r}')
        self.register_channel, self.register_time, self.min_score = register_channel, register_time, float(min_score)

    def __call__(self, assay):
        if "tile" not in assay:
            raise AttributeError("Dataset must contain 'tile' data variable.")
        sizes = assay.data_vars["tile"].sizes
        if self.overlap >= sizes["tile_y"] or self.overlap >= sizes["tile_x"]:
            raise ValueError(f"Overlap ({self.overlap}) must be smaller than tile size "
                             f"({sizes['tile_y']}x{sizes['tile_x']}).")
        hotpath.check_blend(self.blend, self.overlap, sizes["tile_y"], sizes["tile_x"])
        tile = assay.data_vars["tile"].transpose("channel", "time", "tile_row", "tile_col", "tile_y", "tile_x")
        raw = tile.raw
        shaded, lazy = isinstance(raw, shading.LazyShading), isinstance(raw, preprocess.LazyFlatfield)
        tiles = raw.tiles if shaded or lazy else preprocess.to_device(raw)
        # (a fitted shading model never takes the shortcut: it would skip the correction)
        if (not shaded and self.overlap == 0 and sizes["tile_row"] == 1 and sizes["tile_col"] == 1
                and (not lazy or raw.max2 is None) and tiles.is_contiguous()):
            # One tile, nothing to crop and (integer pixels, flat 1, dark 0: LazyFlatfield.max2 is None) nothing to
            # correct: the image IS the tile array -- no pass over it at all (a 4 x 4096^2 assay: 70 us of copying).
            # (and no seam to blend or to register).  The finders take the min / max of the planes they search themselves.
            # The image then shares its memory with the tile array it was given (deliberate differences).
            image = tiles.view(tiles.shape[0], tiles.shape[1], tiles.shape[4], tiles.shape[5])
            assay["image"] = DataArray(image, ("channel", "time", "im_y", "im_x"))
            assay._cache["image_minmax"] = (image.data_ptr(), None)
            return assay
        # register="ncc": one shift per tile, measured on the tiles as this pass will write them (None: nothing moves)
        shifts = self._measure(assay, raw, tiles) if self.register is not None else None
        if shaded:
            # its apply fused with the crop/concat, one launch for all channels
            image, minmax = shading.apply_stitch(tiles, self.overlap, raw.flatfield, raw.darkfield, blend=self.blend,
                                                 shifts=shifts)
        elif lazy:
            image, minmax = hotpath.flatfield_stitch(tiles, self.overlap, raw.flatfield, raw.darkfield, max2=raw.max2,
                                                     blend=self.blend, shifts=shifts)
        else:
            image, minmax = hotpath.flatfield_stitch(tiles, self.overlap, apply_flatfield=False, blend=self.blend,
                                                     shifts=shifts)
        assay["image"] = DataArray(image, ("channel", "time", "im_y", "im_x"))
        assay._cache["image_minmax"] = (image.data_ptr(), minmax)
        return assay

    def _register_planes(self, assay, raw, tiles):
        """The planes that are correlated, (n_tables, R, Cc, ty, tx), as the stitch would write their tiles: a pending
        correction is applied to the selected planes only, through the overlap-0 path (what ``materialize`` does)."""
        c, t, nr, nc, ty, tx = tiles.shape
        ch = self.register_channel
        if ch is None:
            ch = 0
        elif isinstance(ch, str):
            names = assay.coords["channel"].values.tolist() if "channel" in assay.coords else []
            if ch not in names:
                raise ValueError(f"register_channel {ch!r} is not one of the channels {names}")
            ch = names.index(ch)
        if not -c <= int(ch) < c:
            raise ValueError(f"register_channel {ch} outside the {c} channels")
        ch = int(ch) % c
        if self.register_time == "each":
            planes = tiles[ch]
        else:
            if not -t <= int(self.register_time) < t:
                raise ValueError(f"register_time {self.register_time} outside the {t} timepoints")
            at = int(self.register_time) % t
            planes = tiles[ch, at:at + 1]
        planes = planes.contiguous()
        n = planes.shape[0]
        if isinstance(raw, shading.LazyShading):
            out, _ = shading.apply_stitch(planes.reshape(1, n * nr * nc, 1, 1, ty, tx), 0, raw.flatfield[ch:ch + 1],
                                          raw.darkfield[ch:ch + 1], want_minmax=False)
            planes = out.reshape(n, nr, nc, ty, tx)
        elif isinstance(raw, preprocess.LazyFlatfield) and raw.max2 is not None:
            out, _ = hotpath.flatfield_stitch(planes.reshape(n * nr * nc, 1, 1, 1, ty, tx), 0, raw.flatfield, raw.darkfield,
                                              max2=raw.max2, want_minmax=False)
            planes = out.reshape(n, nr, nc, ty, tx)
        return planes

    def _measure(self, assay, raw, tiles):
        """Registers the tiles, leaves ``tile_shift`` / ``seam_shift`` / ``seam_score`` in the dataset (on dimensions of
        their own: ``drop`` and ``restore_format`` leave them alone) and returns the shift tables to stitch with --
        None for all-zero tables, which the plain pass stitches to the same bytes."""
        if self.max_shift > self.overlap // 4:
            raise ValueError(f"max_shift ({self.max_shift}) must not exceed overlap // 4 ({self.overlap // 4})")
        nr, nc = tiles.shape[2:4]
        planes = self._register_planes(assay, raw, tiles)
        if nr * nc > 1:
            found = registration.register_tiles(planes, self.overlap, self.max_shift, self.min_score)
        else:  # no seams: nothing is measured, nothing moves
            found = {"tile_shift": np.zeros((planes.shape[0], 1, 1, 2), dtype=np.int32), "clipped": 0}
        shifts = found["tile_shift"]
        assay["tile_shift"] = DataArray(shifts, ("reg_time", "reg_row", "reg_col", "yx"))
        if "seam_shift" in found:
            assay["seam_shift"] = DataArray(found["seam_shift"], ("reg_time", "seam", "yx"))
            assay["seam_score"] = DataArray(found["seam_score"], ("reg_time", "seam"))
        assay.attrs["tile_shift_clipped"] = int(found["clipped"])
        return shifts if shifts.any() else None

    @registry.components.register("stitch")
    def make(overlap: int = 102, blend=None, register=None, max_shift: int = 8, register_channel=None, register_time=0,
             min_score: float = 0.5):
        return Stitcher(overlap=overlap, blend=blend, register=register, max_shift=max_shift,
                        register_channel=register_channel, register_time=register_time, min_score=min_score)
