"""Plain Python restatement of ``csrc/fingerprint.hip`` (circular fingerprints and their Tanimoto similarity), used by tests
only.  Python integers, no numpy arithmetic, no package import: it shares nothing with the kernels or with
``difflinker_amd.metrics`` but the definitions written in ``include/difflinker_hip.h`` and the mixing function of
``mol_keys_ref``.  numpy only carries the arrays in and out, with the kernels' shapes and dtypes.
"""
import numpy as np

from mol_keys_ref import SEED_COLOUR, M, mix2

MAX_ATOMS, MAX_RADIUS = 256, 4
BONDS_OVERFLOW, TOO_LARGE, BAD_BOND = 1, 4, 8
FIELDS = ('bits', 'n_on', 'n_atoms', 'n_centres', 'status')
NEAREST_FIELDS = ('nn_index', 'nn_common', 'nn_union', 'n_pairs', 'sum_q20')


def on_bits(types, bonds, keep=None, centres=None, radius=2, n_bits=2048):
    """The set of on-bits of one molecule: ``types`` element index per atom, ``bonds`` ``(i, j, order)`` entries (every one of
    them counts, in either orientation), ``keep`` / ``centres`` per atom (``None``: all)."""
    n = len(types)
    keep = [True] * n if keep is None else [bool(k) for k in keep]
    centres = [True] * n if centres is None else [bool(c) for c in centres]
    kept_bonds = [(i, j, o) for i, j, o in bonds if keep[i] and keep[j]]
    c = [mix2(SEED_COLOUR, types[i] + 1) if keep[i] else 0 for i in range(n)]
    bits = set()
    for r in range(radius + 1):
        bits |= {c[i] % n_bits for i in range(n) if keep[i] and centres[i]}
        if r == radius:
            break
        s = [0] * n
        for i, j, o in kept_bonds:
            s[i] = (s[i] + mix2(c[j], o)) & M
            s[j] = (s[j] + mix2(c[i], o)) & M
        c = [mix2(c[i], s[i]) if keep[i] else 0 for i in range(n)]
    return bits


def colours(types, bonds, radius):
    """``c_radius`` of every atom (all kept): what ``mol_keys_ref.colours_and_key`` calls the colours after ``radius`` rounds."""
    n = len(types)
    c = [mix2(SEED_COLOUR, t + 1) for t in types]
    for _ in range(radius):
        s = [0] * n
        for i, j, o in bonds:
            s[i] = (s[i] + mix2(c[j], o)) & M
            s[j] = (s[j] + mix2(c[i], o)) & M
        c = [mix2(c[i], s[i]) for i in range(n)]
    return c


def pack_bits(bits, n_bits):
    words = [0] * (n_bits // 32)
    for k in bits:
        words[k // 32] |= 1 << (k % 32)
    return words


def fingerprints(one_hot, node_mask, bonds, n_bonds_in, status_in, drop_mask=None, centre_mask=None, radius=2, n_bits=2048):
    """Every output of ``dl_fingerprints`` for arrays laid out as ``dl_fingerprint_args`` takes them: ``one_hot [B,N,nf]``,
    masks ``[B,N]``, ``bonds [B,capacity,3]``, ``n_bonds_in`` and ``status_in`` ``[B]``."""
    B, N = node_mask.shape
    capacity = bonds.shape[1]
    W = n_bits // 32
    out = {'bits': np.zeros((B, W), np.uint32), 'n_on': np.zeros(B, np.int32), 'n_atoms': np.zeros(B, np.int32),
           'n_centres': np.zeros(B, np.int32), 'status': np.zeros(B, np.int32)}
    for b in range(B):
        rows = [r for r in range(N) if node_mask[b, r] != 0]
        n = len(rows)
        types = [max(range(one_hot.shape[2]), key=lambda c: (one_hot[b, r, c], -c)) for r in rows]     # the first maximum
        keep = [drop_mask is None or not drop_mask[b, r] != 0 for r in rows]
        centres = [keep[k] and (centre_mask is None or centre_mask[b, r] != 0) for k, r in enumerate(rows)]
        n_in = int(n_bonds_in[b])
        status = int(status_in[b]) | (BONDS_OVERFLOW if n_in > capacity else 0)
        out['n_atoms'][b] = sum(keep)
        if sum(keep) > MAX_ATOMS:
            out['status'][b] = status | TOO_LARGE
            continue
        entries = []
        for i, j, o in bonds[b, :min(max(n_in, 0), capacity)].tolist():
            if 0 <= i < n and 0 <= j < n and i != j and 1 <= o <= 3:
                entries.append((i, j, o))
            else:
                status |= BAD_BOND
        bits = on_bits(types, entries, keep, centres, radius, n_bits)
        out['bits'][b] = pack_bits(bits, n_bits)
        out['n_on'][b], out['n_centres'][b], out['status'][b] = len(bits), sum(centres), status
    return out


def row_ints(bits):
    """The rows of a ``[M,W]`` array of 32-bit words as Python integers."""
    return [sum(int(w) << (32 * k) for k, w in enumerate(row)) for row in np.asarray(bits).astype(np.uint32).tolist()]


def popcount(v):
    return bin(v).count('1')


def tanimoto_nearest(a_bits, b_bits, a_offsets=None, b_offsets=None, exclude_diagonal=False, want_sum=True):
    """Every output of ``dl_tanimoto_nearest``: ``a_bits [Ma,W]``, ``b_bits [Mb,W]``, offsets ``[G+1]`` (``None``: one group
    over everything; an empty list: no group).  ``sum_q20`` is ``None`` without ``want_sum``."""
    a, b = row_ints(a_bits), row_ints(b_bits)
    Ma, Mb = len(a), len(b)
    if a_offsets is None:
        a_offsets, b_offsets = [0, Ma], [0, Mb]
    a_off = [min(max(int(v), 0), Ma) for v in a_offsets]
    b_off = [min(max(int(v), 0), Mb) for v in b_offsets]
    pa, pb = [popcount(v) for v in a], [popcount(v) for v in b]
    out = {'nn_index': np.full(Ma, -1, np.int32), 'nn_common': np.zeros(Ma, np.int32), 'nn_union': np.zeros(Ma, np.int32),
           'n_pairs': np.zeros(Ma, np.int32), 'sum_q20': np.zeros(Ma, np.uint64) if want_sum else None}
    for g in range(len(a_off) - 1):
        for i in range(a_off[g], a_off[g + 1]):
            best, total, pairs = None, 0, 0
            for j in range(b_off[g], b_off[g + 1]):
                if exclude_diagonal and j == i:
                    continue
                c = popcount(a[i] & b[j])
                u = pa[i] + pb[j] - c
                num, den = (c, u) if u else (1, 1)
                pairs += 1
                total += (c << 20) // u if u else 1 << 20
                if best is None or num * best[1] > best[0] * den:
                    best = (num, den, j, c, u)
            out['n_pairs'][i] = pairs
            if best is not None:
                out['nn_index'][i], out['nn_common'][i], out['nn_union'][i] = best[2], best[3], best[4]
            if want_sum:
                out['sum_q20'][i] = total
    return out


def ring(n, first=0):
    return [(first + k, first + (k + 1) % n) for k in range(n)]


# the hand molecules of the pinned values: type index 0 = C, 2 = N
BENZENE = ([0] * 6, [(i, j, 1 + k % 2) for k, (i, j) in enumerate(ring(6))])
TOLUENE = ([0] * 7, BENZENE[1] + [(0, 6, 1)])
HEXANE = ([0] * 6, [(k, k + 1, 1) for k in range(5)])
PYRIDINE = ([2] + [0] * 5, BENZENE[1])
