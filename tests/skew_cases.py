"""The tilted chips and the planes without a grid that the skew tests share: name -> (plane, feature,
tilt), built once.  ``tilt`` is what ``rotate_ref.rotate`` turned the chip by, so the estimate is minus it; None for the
planes that hold no grid."""
import functools

import numpy as np

import rotate_ref as rr
from synth import draw_chip, vignette

CHIP_TILTS = (4.0, -2.3, 0.0, 7.77, -9.6)


def ten_by_ten(tilt):
    return rr.rotate(draw_chip((10, 10), 20), tilt)


def noisy_chip():
    """The 10 x 10 chip at 4 degrees on a lit, sloping, noisy background under a vignette, as uint16."""
    rng = np.random.default_rng(34)
    chip = ten_by_ten(4.0).astype(np.float64)
    h, w = chip.shape
    lit = chip + 300.0 + np.linspace(0.0, 3000.0, w)[None, :] + rng.normal(0.0, 30.0, size=(h, w))
    return np.clip(np.rint(lit * vignette((h, w), 0.4, np.float64)), 0, 65535).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def chips():
    out = {f"10x10 at {t:g}": (ten_by_ten(t), 16, t) for t in CHIP_TILTS}
    out["noisy 10x10 at 4"] = (noisy_chip(), 16, 4.0)
    out["6x12 with blanks at 3.1"] = (rr.rotate(draw_chip((6, 12), 20, blanks=((0, 0), (2, 5), (5, 11))), 3.1), 16, 3.1)
    out["3x3 at -5.2"] = (rr.rotate(draw_chip((3, 3), 20), -5.2), 16, -5.2)
    out["small 3x3 at -5.2"] = (rr.rotate(draw_chip((3, 3), 12, 40, 40), -5.2), 10, -5.2)
    out["4x5 at 2.9"] = (rr.rotate(draw_chip((4, 5), 14, 47, 53), 2.9), 12, 2.9)
    out["float32 10x10 at 4"] = (ten_by_ten(4.0).astype(np.float32) / np.float32(7.0), 16, 4.0)
    return out


@functools.lru_cache(maxsize=None)
def blanks():
    rng = np.random.default_rng(35)
    return {"uniform noise": (rng.integers(0, 60000, size=(300, 300)).astype(np.uint16), 16, None),
            "flat with noise": (np.rint(1000.0 + rng.normal(0.0, 30.0, size=(300, 300))).astype(np.uint16), 16, None)}


def tolerance(plane):
    """One pixel at the rim of the inscribed disk, in degrees."""
    return float(np.degrees(2.0 / min(plane.shape)))
