"""The clash rule of ``include/difflinker_hip.h`` (``dl_clash_scores``) restated in numpy float32 - a test helper, the ground
truth of ``tests/test_gpu_clash.py``.  The reference repository has no code for this score, so there is nothing to port: the
rule is written down in the header and here, with the same operations in the same order, one fp32 rounding each:

    dx = xq - xt;  d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
    clash   : d2 < t * t and t > 0,   t = threshold[query type][target type]
    contact : d2 < c * c

numpy rounds every float32 operation to nearest and fuses nothing, so counts and minima come out with the kernel's bits.

Worked by hand (``test_clash_host.test_reference_on_a_case_worked_by_hand``): queries C at (0,0,0) and O at (10,0,0); targets N
at (2,0,0) and C at (0,3,0); thresholds all 2.5, cut-off 4.  C-N: d2 = 4 < 6.25, a clash and a contact.  C-C: d2 = 9, a
contact only (9 < 16).  O-N: d2 = 64, O-C: d2 = 109, nothing.  So n_clashes 1, n_clash_atoms 1, n_contacts 2, min_dist2 4,
atom_clashes [1, 0], atom_min_dist2 [4, 64]."""
import numpy as np

NONFINITE, TOO_LARGE, BAD_TYPE = 1, 2, 4
MAX_QUERY = 1024
F = np.float32


def first_maximum(rows):
    """Index of the first largest entry of every row, found as the kernel finds it: a later entry wins only when greater."""
    rows = np.asarray(rows, dtype=F)
    best = np.zeros(len(rows), dtype=np.int64)
    vmax = rows[:, 0].copy()
    for c in range(1, rows.shape[1]):
        better = rows[:, c] > vmax
        best[better] = c
        vmax[better] = rows[better, c]
    return best


def dist2(q, t):
    """``[nq, nt]`` squared distances of fp32 ``q [nq,3]`` and ``t [nt,3]``: five fp32 operations per pair in the rule's order."""
    with np.errstate(over='ignore', invalid='ignore'):
        dx = q[:, None, 0] - t[None, :, 0]
        dy = q[:, None, 1] - t[None, :, 1]
        dz = q[:, None, 2] - t[None, :, 2]
        return ((dx * dx) + (dy * dy)) + (dz * dz)


def clash_scores(x, one_hot, query_mask, threshold, target_mask=None, protein_x=None, protein_type=None, contact_cutoff=4.0):
    """Every output of ``dl_clash_scores`` as numpy arrays in a dict, for ``x [B,N,3]``, ``one_hot [B,N,nf]``, masks ``[B,N]``,
    ``threshold [nf,nf]`` and the shared list ``protein_x [M,3]``, ``protein_type [M]``."""
    x, one_hot = np.asarray(x, dtype=F), np.asarray(one_hot, dtype=F)
    B, N, nf = one_hot.shape
    qm = np.asarray(query_mask, dtype=F).reshape(B, N) != 0
    tm = np.zeros((B, N), dtype=bool) if target_mask is None else np.asarray(target_mask, dtype=F).reshape(B, N) != 0
    tm = tm & ~qm                                                       # a row in both masks is a query only
    threshold = np.asarray(threshold, dtype=F).reshape(nf, nf)
    with np.errstate(over='ignore', invalid='ignore'):
        t2 = np.where(threshold > 0, threshold * threshold, F(0)).astype(F)   # d2 >= 0: `d2 < 0` never holds
        c2 = F(contact_cutoff) * F(contact_cutoff)
    M = 0 if protein_type is None else len(protein_type)
    px = np.zeros((0, 3), dtype=F) if M == 0 else np.asarray(protein_x, dtype=F).reshape(M, 3)
    pt = np.zeros(0, dtype=np.int64) if M == 0 else np.asarray(protein_type, dtype=np.int64)
    typed = (pt >= 0) & (pt < nf)
    shared_status = 0 if typed.all() else BAD_TYPE
    px, pt = px[typed], pt[typed]
    if not np.isfinite(px).all():
        shared_status |= NONFINITE
    out = {'n_query': np.zeros(B, np.int32), 'n_target': np.zeros(B, np.int32), 'n_clashes': np.zeros(B, np.int32),
           'n_clash_atoms': np.zeros(B, np.int32), 'n_contacts': np.zeros(B, np.int32), 'min_dist2': np.full(B, np.inf, F),
           'status': np.zeros(B, np.int32), 'atom_clashes': np.zeros((B, N), np.int32),
           'atom_min_dist2': np.full((B, N), np.inf, F)}
    for b in range(B):
        q_rows, t_rows = np.nonzero(qm[b])[0], np.nonzero(tm[b])[0]
        if len(q_rows) > MAX_QUERY:
            status = TOO_LARGE                                          # decided first; the molecule is not looked at further
        else:
            status = shared_status
            q, t = x[b, q_rows], np.concatenate([x[b, t_rows], px])
            if not (np.isfinite(q).all() and np.isfinite(t).all()):
                status |= NONFINITE
        out['status'][b] = status
        if status & (NONFINITE | TOO_LARGE):
            out['min_dist2'][b] = np.nan
            out['atom_min_dist2'][b, q_rows] = np.nan
            continue
        qa = first_maximum(one_hot[b, q_rows]) if len(q_rows) else np.zeros(0, np.int64)
        tb = np.concatenate([first_maximum(one_hot[b, t_rows]) if len(t_rows) else np.zeros(0, np.int64), pt])
        out['n_query'][b], out['n_target'][b] = len(q_rows), len(tb)
        if len(qa) == 0 or len(tb) == 0:
            continue
        d2 = dist2(q, t)
        clash = d2 < t2[qa[:, None], tb[None, :]]
        out['n_clashes'][b] = clash.sum()
        out['n_clash_atoms'][b] = clash.any(1).sum()
        out['n_contacts'][b] = (d2 < c2).sum()
        out['min_dist2'][b] = d2.min()
        out['atom_clashes'][b, q_rows] = clash.sum(1)
        out['atom_min_dist2'][b, q_rows] = d2.min(1)
    return out
