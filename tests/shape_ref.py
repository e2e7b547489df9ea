"""The shape rule of ``include/difflinker_hip.h`` (``dl_shape_scores``) restated in numpy float32 - a test helper, the ground
truth of ``tests/test_gpu_shape.py``.  The rule is this project's own (after RDKit's defaults: spacing 0.5, vdW scale 0.8, two
layers of 0.25; NOT RDKit's grid or numbers), so there is nothing to port: it is written down in the header and here, with the
same operations in the same order, one fp32 rounding each:

    p = (0.5f*i, 0.5f*j, 0.5f*k);  dx = px - xa;  d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
    an atom of type t gives the point  (d2 < r2[t][0]) + (d2 < r2[t][1]) + (d2 < r2[t][2])
    level of a point for a molecule = the maximum of that over its participating atoms
    vol = sum of levels, vol_min = sum of min(level_A, level_B), core = points at level 3

numpy rounds every float32 operation to nearest and fuses nothing, and every output is an integer sum, so the numbers come
out as the kernel's.  ``shape_scores`` keeps one dense ``uint8`` array of levels per molecule over a box of its own choosing
(the lattice extent of both molecules, padded by what the largest radius reaches plus two steps) and visits, per atom, the
cube of lattice points that atom can reach; ``levels_dense`` evaluates every atom at every point of a box instead, and
``tests/test_shape_host.py`` holds the two against each other.

Worked by hand (``test_shape_host.test_reference_reproduces_the_numbers_worked_by_hand``), with the default table:
  * one C at the origin: r = 1.36, 1.61, 1.86, r2 = 1.8496001, 2.5921001, 3.4596; vol = 431, core = 81
  * one O at (1,0,0): vol = 321, core = 57
  * C at the origin against that O: vol_min = 196, core_both = 27
  * C at the origin against C at (0.25,0,0): vol_b = 460, core_b = 94, vol_min = 394, core_both = 77 - the lattice is fixed in
    the frame of the coordinates, so a shift below its spacing changes the counts
  * C at the origin against C at (5,0,0): vol_min = 0"""
import numpy as np

NONFINITE, OUT_OF_RANGE, TOO_LARGE = 1, 2, 4
COORD_MAX, EXTENT_MAX = 4096.0, 240
F = np.float32
VDW = (1.70, 1.52, 1.55, 1.47, 1.80, 1.75, 1.85, 1.98, 1.80)         # Bondi; C O N F S Cl Br I P
FIELDS = ('vol_a', 'vol_b', 'vol_min', 'core_a', 'core_b', 'core_both', 'n_a', 'n_b', 'status')


def radius_table(n_types=9, scale=0.8, step=0.25):
    """``r2[type][k]``: ``scale * vdw + k * step`` in fp64, rounded to fp32 once, squared in fp32."""
    r = np.array([[scale * VDW[t] + k * step for k in range(3)] for t in range(n_types)], dtype=np.float64).astype(F)
    return r * r


def first_maximum(rows):
    """Index of the first largest entry of every row: a later entry wins only when greater."""
    rows = np.asarray(rows, dtype=F)
    best = np.zeros(len(rows), dtype=np.int64)
    vmax = rows[:, 0].copy()
    for c in range(1, rows.shape[1]):
        better = rows[:, c] > vmax
        best[better] = c
        vmax[better] = rows[better, c]
    return best


def point_levels(x, r2, i, j, k):
    """Level one atom at fp32 ``x [3]`` with squared radii ``r2 [3]`` gives the lattice points ``(i, j, k)`` (integer arrays
    that broadcast against each other)."""
    dx = F(0.5) * i.astype(F) - x[0]
    dy = F(0.5) * j.astype(F) - x[1]
    dz = F(0.5) * k.astype(F) - x[2]
    d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
    return ((d2 < r2[0]).astype(np.uint8) + (d2 < r2[1])) + (d2 < r2[2])


def levels_dense(x, types, r2, lo, hi):
    """``uint8`` levels of a molecule on the box ``lo .. hi`` (inclusive lattice indices per axis), every atom at every point."""
    axes = [np.arange(lo[d], hi[d] + 1) for d in range(3)]
    i, j, k = axes[0][:, None, None], axes[1][None, :, None], axes[2][None, None, :]
    level = np.zeros([len(a) for a in axes], dtype=np.uint8)
    for p, t in zip(np.asarray(x, dtype=F), types):
        level = np.maximum(level, point_levels(p, r2[t], i, j, k))
    return level


def levels_by_atom(x, types, r2, lo, hi, reach):
    """The same array, each atom visiting only the cube ``floor(2x) - reach .. floor(2x) + 1 + reach`` around it."""
    level = np.zeros([hi[d] - lo[d] + 1 for d in range(3)], dtype=np.uint8)
    for p, t in zip(np.asarray(x, dtype=F), types):
        c = np.floor(F(2) * p).astype(np.int64)
        first, last = np.maximum(c - reach, lo), np.minimum(c + 1 + reach, hi)
        axes = [np.arange(first[d], last[d] + 1) for d in range(3)]
        sub = tuple(slice(first[d] - lo[d], last[d] - lo[d] + 1) for d in range(3))
        got = point_levels(p, r2[t], axes[0][:, None, None], axes[1][None, :, None], axes[2][None, None, :])
        level[sub] = np.maximum(level[sub], got)
    return level


def pair_scores(xa, ta, xb, tb, r2, dense=False):
    """The six sums and the status of one pair whose participating atoms are ``xa [na,3]`` of types ``ta`` and ``xb``, ``tb``."""
    both = np.concatenate([xa, xb]).astype(F)
    if not np.isfinite(both).all():
        return (0,) * 6, NONFINITE
    if (np.abs(both) > F(COORD_MAX)).any():
        return (0,) * 6, OUT_OF_RANGE
    if len(both) == 0:
        return (0,) * 6, 0
    cells = np.floor(F(2) * both).astype(np.int64)
    lo, hi = cells.min(0), cells.max(0)
    if ((hi - lo) > EXTENT_MAX).any():
        return (0,) * 6, TOO_LARGE
    reach = int(np.ceil(2.0 * np.sqrt(np.float64(r2.max())))) + 2
    lo, hi = lo - reach, hi + 1 + reach
    if dense:
        la, lb = levels_dense(xa, ta, r2, lo, hi), levels_dense(xb, tb, r2, lo, hi)
    else:
        la, lb = levels_by_atom(xa, ta, r2, lo, hi, reach), levels_by_atom(xb, tb, r2, lo, hi, reach)
    count = lambda v: int(v.sum(dtype=np.int64))           # noqa: E731
    return (count(la), count(lb), count(np.minimum(la, lb)), count(la == 3), count(lb == 3), count((la == 3) & (lb == 3))), 0


def shape_scores(x_a, one_hot_a, mask_a, x_b, one_hot_b, mask_b, r2=None, dense=False):
    """Every output of ``dl_shape_scores`` as int32 arrays ``[B]`` in a dict, for ``x_a [B,Na,3]``, ``one_hot_a [B,Na,nf]``,
    ``mask_a [B,Na]``, the same for B, and ``r2 [nf,3]`` (default: ``radius_table(nf)``)."""
    x_a, x_b = np.asarray(x_a, dtype=F), np.asarray(x_b, dtype=F)
    one_hot_a, one_hot_b = np.asarray(one_hot_a, dtype=F), np.asarray(one_hot_b, dtype=F)
    B, Na, nf = one_hot_a.shape
    Nb = one_hot_b.shape[1]
    r2 = radius_table(nf) if r2 is None else np.asarray(r2, dtype=F).reshape(nf, 3)
    ma = np.asarray(mask_a, dtype=F).reshape(B, Na) != 0
    mb = np.asarray(mask_b, dtype=F).reshape(B, Nb) != 0
    out = {name: np.zeros(B, np.int32) for name in FIELDS}
    for b in range(B):
        xa, xb = x_a[b][ma[b]], x_b[b][mb[b]]
        ta = first_maximum(one_hot_a[b][ma[b]]) if len(xa) else np.zeros(0, np.int64)
        tb = first_maximum(one_hot_b[b][mb[b]]) if len(xb) else np.zeros(0, np.int64)
        with np.errstate(invalid='ignore', over='ignore'):
            sums, status = pair_scores(xa, ta, xb, tb, r2, dense)
        out['status'][b] = status
        if status:
            continue
        for name, v in zip(FIELDS[:6], sums):
            out[name][b] = v
        out['n_a'][b], out['n_b'][b] = len(xa), len(xb)
    return out
