"""The pin of the symmetry-aware RMSD tests: a helper, not a test.

RDKit is not available where this suite runs, so ``rdMolAlign.GetBestRMS`` (the reference's compute_metrics.py:366-402) is
restated here by other means than the code under test, in fp64 numpy:

* isomorphisms by plain recursion over the atoms in their given order, constrained by element, degree and the order of
  every bond to an atom already placed - no colours, no visiting order, nothing shared with ``difflinker_amd.metrics``;
* the alignment by Kabsch: SVD of the 3x3 covariance with the determinant correction, so proper rotations only, and the
  residual summed directly after rotating - not the quaternion eigenvalue problem the kernel solves.
"""
import numpy as np


def adjacency(n, bonds):
    adj = [dict() for _ in range(n)]
    for i, j, order in bonds:
        adj[i][j] = order
        adj[j][i] = order
    return adj


def isomorphisms(types_a, bonds_a, types_b, bonds_b, limit=None):
    """Every map ``image`` (atom k of a -> atom image[k] of b) that is a bijection and keeps elements and bond orders."""
    n = len(types_a)
    if n != len(types_b) or len(bonds_a) != len(bonds_b):
        return []
    adj_a, adj_b = adjacency(n, bonds_a), adjacency(n, bonds_b)
    found, image, used = [], [-1] * n, [False] * n

    def place(k):
        if limit is not None and len(found) >= limit:
            return
        if k == n:
            found.append(list(image))
            return
        for v in range(n):
            if used[v] or types_b[v] != types_a[k] or len(adj_b[v]) != len(adj_a[k]):
                continue
            if any(image[w] >= 0 and adj_b[v].get(image[w]) != o for w, o in adj_a[k].items()):
                continue
            image[k], used[v] = v, True
            place(k + 1)
            image[k], used[v] = -1, False

    place(0)
    return found


def is_isomorphism(image, types_a, bonds_a, types_b, bonds_b):
    n = len(types_a)
    if sorted(image) != list(range(n)) or len(bonds_a) != len(bonds_b):
        return False
    adj_b = adjacency(n, bonds_b)
    return all(types_a[k] == types_b[image[k]] for k in range(n)) and \
        all(adj_b[image[i]].get(image[j]) == o for i, j, o in bonds_a)


def kabsch_rmsd(a, b):
    """RMSD of the point sets ``a`` and ``b`` ([n, 3], row k of one against row k of the other) after the best rigid motion
    of ``a`` onto ``b`` with a proper rotation."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    a = a - a.mean(0)
    b = b - b.mean(0)
    u, _, vt = np.linalg.svd(a.T @ b)
    d = np.sign(np.linalg.det(u @ vt))
    if d == 0:
        d = 1.0
    rot = u @ np.diag([1.0, 1.0, d]) @ vt                             # rows of a times rot land on b
    return float(np.sqrt((((a @ rot) - b) ** 2).sum() / len(a)))


def best_rmsd(a, b, maps):
    """``(rmsd, index)`` of the best of ``maps``, the lowest index among equal values."""
    b = np.asarray(b, dtype=np.float64)
    values = [kabsch_rmsd(a, b[list(image)]) for image in maps]
    k = int(np.argmin(values))
    return values[k], k
