"""The interaction rule of ``include/difflinker_hip.h`` (``dl_interaction_types`` and ``dl_interaction_scores``) restated in
numpy - a test helper, the ground truth of ``tests/test_gpu_interaction.py``.  The reference repository has no code for this
score, so there is nothing to port: the rule is written down in the header and here, with the same operations in the same order.

Typing, fp32:   neighbours when ``100 * sqrt(dx*dx + dy*dy + dz*dz) < table[element of the higher row][of the lower row]``
                (strict, as ``bonds.hip``), the oxygen's ``d2 = ((dx*dx) + (dy*dy)) + (dz*dz) >= 1.6875``.
Scores, fp64:   from the fp32 coordinates widened to fp64, ``d2`` in the same order, ``d2 < 64`` strict,
                ``s = sqrt(d2) - (R[a] + R[b])``, the five terms, each rounded to fixed point with ``np.rint(term * 2^32)``;
                all sums are int64 sums.

numpy rounds every operation to nearest and fuses nothing.  Its ``exp`` may differ from the device's in the last places, which
moves a pair's rounded Gaussian by at most one unit; everything else has the kernel's bits."""
import numpy as np

import clash_ref

HYDROPHOBIC, DONOR, ACCEPTOR = 16, 32, 64
NONFINITE, TOO_LARGE, BAD_TYPE, UNTYPED = 1, 2, 4, 8
MAX_QUERY = 1024
TERMS = ('gauss1', 'gauss2', 'repulsion', 'hydrophobic', 'hbond')
ONE = 4294967296.0                                                     # 2^32
C, O, N, F_, S, CL, BR, I, P = range(9)                                # the project's atom order
F = np.float32
first_maximum = clash_ref.first_maximum


def flags_of(elem, deg, hetero, first_d2):
    """``xs_type`` of one atom from its element, its neighbour count, whether a neighbour is no carbon, and the fp32 squared
    distance of its first neighbour (read when ``deg == 1`` only)."""
    flags = 0
    if elem == C:
        flags = 0 if hetero else HYDROPHOBIC
    elif elem in (F_, CL, BR, I):
        flags = HYDROPHOBIC
    elif elem == N:
        flags = DONOR if deg < 3 else 0
    elif elem == O:
        flags = ACCEPTOR | (DONOR if deg == 0 or (deg == 1 and first_d2 >= F(1.6875)) else 0)
    return int(elem) | flags


def interaction_types(x, one_hot, group, table):
    """``(xs_type [B,N] int32, status [B] int32)`` for ``x [B,N,3]``, ``one_hot [B,N,nf]``, ``group [B,N]`` (0 = not typed) and
    the single-bond bounds ``table [nf,nf]`` in pm."""
    x, one_hot = np.asarray(x, dtype=F), np.asarray(one_hot, dtype=F)
    B, n_rows, nf = one_hot.shape
    group = np.asarray(group).reshape(B, n_rows).astype(np.int64)
    table = np.asarray(table, dtype=F).reshape(nf, nf)
    xs = np.full((B, n_rows), -1, np.int32)
    status = np.zeros(B, np.int32)
    for b in range(B):
        rows = np.nonzero(group[b])[0]
        if len(rows) == 0:
            continue
        p = x[b, rows]
        if not np.isfinite(p).all():
            status[b] = NONFINITE
            continue
        e, g = first_maximum(one_hot[b, rows]), group[b, rows]
        dx, dy, dz = (p[:, None, k] - p[None, :, k] for k in range(3))
        d = F(100) * np.sqrt(dx * dx + dy * dy + dz * dz)
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        higher = np.arange(len(rows))[:, None] > np.arange(len(rows))[None, :]
        bound = np.where(higher, table[e[:, None], e[None, :]], table[e[None, :], e[:, None]])
        nb = (d < bound) & (g[:, None] == g[None, :]) & ~np.eye(len(rows), dtype=bool)
        deg = nb.sum(1)
        hetero = (nb & (e[None, :] != C)).any(1)
        first = nb.argmax(1)
        for k, r in enumerate(rows):
            xs[b, r] = flags_of(e[k], deg[k], hetero[k], d2[k, first[k]])
    return xs, status


def fixed(term):
    return np.rint(np.asarray(term, dtype=np.float64) * ONE).astype(np.int64)


def pair_terms(s, hydrophobic, hbond):
    """``[5, ...]`` int64: the fixed-point terms of pairs at surface distance ``s`` (fp64), ``hydrophobic`` / ``hbond`` saying
    whether the two atoms' types allow that term."""
    s = np.asarray(s, dtype=np.float64)
    u, v = s / 0.5, (s - 3.0) / 2.0
    zero = np.zeros_like(s)
    return np.stack([fixed(np.exp(-(u * u))), fixed(np.exp(-(v * v))), fixed(np.where(s < 0, s * s, zero)),
                     fixed(np.where(hydrophobic, np.where(s < 0.5, 1.0, np.where(s < 1.5, 1.5 - s, zero)), zero)),
                     fixed(np.where(hbond, np.where(s < -0.7, 1.0, np.where(s < 0, -s / 0.7, zero)), zero))])


def interaction_scores(x, xs_type, query_mask, radius, target_mask=None, protein_x=None, protein_xs=None):
    """Every output of ``dl_interaction_scores`` as numpy arrays in a dict, for ``x [B,N,3]``, ``xs_type [B,N]``, masks
    ``[B,N]``, ``radius [nf]`` (fp64) and the shared list ``protein_x [M,3]``, ``protein_xs [M]``."""
    x = np.asarray(x, dtype=F)
    B, n_rows = x.shape[:2]
    xs_type = np.asarray(xs_type).reshape(B, n_rows).astype(np.int64)
    radius = np.asarray(radius, dtype=np.float64)
    nf = len(radius)
    qm = np.asarray(query_mask, dtype=F).reshape(B, n_rows) != 0
    tm = np.zeros((B, n_rows), dtype=bool) if target_mask is None else np.asarray(target_mask, dtype=F).reshape(B, n_rows) != 0
    tm = tm & ~qm                                                       # a row in both masks is a query only
    M = 0 if protein_xs is None else len(protein_xs)
    px = np.zeros((0, 3), dtype=F) if M == 0 else np.asarray(protein_x, dtype=F).reshape(M, 3)
    pxs = np.zeros(0, dtype=np.int64) if M == 0 else np.asarray(protein_xs, dtype=np.int64)
    usable = lambda t: (t >= 0) & ((t & 15) < nf)                       # noqa: E731
    shared_status = 0 if usable(pxs).all() else BAD_TYPE
    px, pxs = px[usable(pxs)], pxs[usable(pxs)]
    if not np.isfinite(px).all():
        shared_status |= NONFINITE
    i32 = lambda: np.zeros(B, np.int32)                                 # noqa: E731
    out = {'n_query': i32(), 'n_target': i32(), 'n_pairs': i32(), 'n_hbonds': i32(), 'n_hydrophobic': i32(),
           'terms': np.zeros((B, 5), np.int64), 'status': i32(), 'atom_terms': np.zeros((B, n_rows, 5), np.int64)}
    for b in range(B):
        q_rows, t_rows = np.nonzero(qm[b])[0], np.nonzero(tm[b])[0]
        if len(q_rows) > MAX_QUERY:
            out['status'][b] = TOO_LARGE                                # decided first; the molecule is not looked at further
            continue
        status = shared_status
        qs, own = xs_type[b, q_rows], xs_type[b, t_rows]
        if not (usable(qs).all() and usable(own).all()):
            status |= UNTYPED
        t_rows = t_rows[usable(own)]                                    # (an untyped row's coordinates are not looked at)
        q, t = x[b, q_rows], np.concatenate([x[b, t_rows], px])
        ts = np.concatenate([xs_type[b, t_rows], pxs])
        if not (np.isfinite(q).all() and np.isfinite(t).all()):
            status |= NONFINITE
        out['status'][b] = status
        if status & (NONFINITE | UNTYPED):
            continue
        out['n_query'][b], out['n_target'][b] = len(q_rows), len(ts)
        if len(qs) == 0 or len(ts) == 0:
            continue
        q, t = q.astype(np.float64), t.astype(np.float64)
        dx, dy, dz = (q[:, None, k] - t[None, :, k] for k in range(3))
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        inside = d2 < 64.0
        s = np.sqrt(d2) - (radius[qs & 15][:, None] + radius[ts & 15][None, :])
        hyd = ((qs[:, None] & ts[None, :]) & HYDROPHOBIC) != 0
        hb = (((qs[:, None] & DONOR) != 0) & ((ts[None, :] & ACCEPTOR) != 0)) | \
            (((qs[:, None] & ACCEPTOR) != 0) & ((ts[None, :] & DONOR) != 0))
        terms = pair_terms(s, hyd, hb) * inside[None]
        out['n_pairs'][b] = inside.sum()
        out['n_hydrophobic'][b] = (inside & hyd & (s < 1.5)).sum()
        out['n_hbonds'][b] = (inside & hb & (s < 0)).sum()
        out['terms'][b] = terms.sum((1, 2))
        out['atom_terms'][b, q_rows] = terms.sum(2).T
    return out


def score(terms, weights):
    """The weighted score of fixed-point term sums ``[..., 5]`` in fp64, the terms taken in order."""
    terms = np.asarray(terms)
    total = np.zeros(terms.shape[:-1])
    for k, w in enumerate(weights):
        total = total + w * terms[..., k].astype(np.float64)
    return total / ONE
