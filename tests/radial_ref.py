"""The contract of mg_roi_radial_profile (include/magnify_hip.h) restated in plain Python: loops over pixels, Python
integers for the squared distances and for the integer sums, ``math.fsum`` for float sums.  Shares no code with the
product.

With S = 16, centres {cy, cx} and edges integers in 1/16 pixel: pixel (i, j) has d2 = (i S - cy)^2 + (j S - cx)^2 and
belongs to ring k iff edges[k]^2 <= d2 < edges[k + 1]^2 (on an edge: the outer ring; inside edges[0] or from the last
edge on: none).  It takes part iff its mask byte is non-zero (no mask: every pixel) and its value is not NaN.  The kernel
clamps a centre into [-1024 S, 2048 S]."""
import bisect
import math
from fractions import Fraction

import numpy as np

S = 16
CENTRE_MIN, CENTRE_MAX = -1024 * S, 2048 * S


def ring_map(L, cy, cx, edges):
    """Ring index of every pixel of an L x L window as a list of lists, -1 where the pixel belongs to none."""
    cy, cx = min(max(int(cy), CENTRE_MIN), CENTRE_MAX), min(max(int(cx), CENTRE_MIN), CENTRE_MAX)
    e2 = [int(e) * int(e) for e in edges]
    out = []
    for i in range(L):
        row = []
        for j in range(L):
            d2 = (i * S - cy) ** 2 + (j * S - cx) ** 2
            k = bisect.bisect_right(e2, d2) - 1  # the last edge with e2[k] <= d2 (the edges increase strictly)
            row.append(k if 0 <= k < len(e2) - 1 else -1)
        out.append(row)
    return out


def _ieee_sum(values):
    """fsum where everything is finite; with infinities under the sum, what any order of IEEE additions gives."""
    pos, neg = any(v == math.inf for v in values), any(v == -math.inf for v in values)
    if pos or neg:
        return math.nan if pos and neg else (math.inf if pos else -math.inf)
    return math.fsum(values)


def _exact_sum_of_squares(values):
    """The correctly rounded sum of the exact squares (rational arithmetic); inf where a value is infinite."""
    if any(math.isinf(v) for v in values):
        return math.inf
    return float(sum((Fraction(v) * Fraction(v) for v in values), Fraction(0)))


def profile(roi, mask, centre_q, edges_q):
    """roi (M, C, T, L, L) of uint8 / uint16 / float32 / float64; mask None or (M, T', L, L); centre_q integers
    (M, T'', 2) = {cy, cx}; T', T'' = 1 or T; edges_q integers (R + 1,).
    -> dict: count int64 (M, C, T, R); moments float64 (M, C, T, R, 2), the correctly rounded exact {sum x, sum x^2};
    mag float64 (M, C, T, R, 2) = {sum |x|, sum x^2} of the finite values: what the error bounds of a float sum scale
    with; rings int (M, T, L, L): the ring of every pixel, -1 for none (mask not applied)."""
    roi = np.asarray(roi)
    M, C, T, L, _ = roi.shape
    R = len(edges_q) - 1
    centre_q = np.asarray(centre_q).reshape(M, -1, 2)
    integer = roi.dtype.kind == "u"
    count = np.zeros((M, C, T, R), dtype=np.int64)
    moments = np.zeros((M, C, T, R, 2), dtype=np.float64)
    mag = np.zeros((M, C, T, R, 2), dtype=np.float64)
    rings = np.full((M, T, L, L), -1, dtype=np.int64)
    for g in range(M):
        for t in range(T):
            cy, cx = centre_q[g, t if centre_q.shape[1] > 1 else 0]
            rm = ring_map(L, cy, cx, edges_q)
            rings[g, t] = np.array(rm).reshape(L, L)
            mk = None if mask is None else np.asarray(mask)[g, t if np.asarray(mask).shape[1] > 1 else 0]
            for c in range(C):
                win = roi[g, c, t].tolist()  # Python ints / floats (float32 values exactly, as float64)
                per_ring = [[] for _ in range(R)]
                for i in range(L):
                    for j in range(L):
                        k = rm[i][j]
                        if k < 0 or (mk is not None and not mk[i, j]):
                            continue
                        x = win[i][j]
                        if x != x:
                            continue
                        per_ring[k].append(x)
                for k, xs in enumerate(per_ring):
                    count[g, c, t, k] = len(xs)
                    if integer:
                        s1, s2 = sum(xs), sum(x * x for x in xs)  # Python integers: exact
                        moments[g, c, t, k] = float(s1), float(s2)  # (int -> float rounds correctly)
                        mag[g, c, t, k] = moments[g, c, t, k]
                    else:
                        moments[g, c, t, k, 0] = _ieee_sum(xs)
                        moments[g, c, t, k, 1] = _exact_sum_of_squares(xs)
                        fin = [x for x in xs if math.isfinite(x)]
                        mag[g, c, t, k] = math.fsum(abs(x) for x in fin), _exact_sum_of_squares(fin)
    return {"count": count, "moments": moments, "mag": mag, "rings": rings}
