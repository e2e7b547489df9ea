"""Plain Python restatement of ``csrc/mol_keys.hip`` (colour refinement with 64-bit integers), used by tests only.

Python integers masked to 64 bits, no numpy arithmetic, no package import: it shares nothing with the kernel or with
``difflinker_amd.metrics`` but the definition written in the header of ``mol_keys.hip``.
"""
M = (1 << 64) - 1
SEED_COLOUR, SEED_KEY, MIX_B = 0x243F6A8885A308D3, 0x13198A2E03707344, 0xD6E8FEB86659FD93


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def mix2(a, b):
    return mix64((a + b * MIX_B) & M)


def signed(v):
    """The int64 a torch tensor shows for the 64 bits of ``v``."""
    return v - (1 << 64) if v >> 63 else v


def colours_and_key(types, bonds, keep=None):
    """``types``: element index per atom; ``bonds``: ``(i, j, order)``; ``keep``: per atom, False = dropped.
    Returns ``(colours, key, n_atoms, n_bonds)``; a dropped atom's colour is 0."""
    n = len(types)
    keep = [True] * n if keep is None else [bool(k) for k in keep]
    kept_bonds = [(i, j, o) for i, j, o in bonds if keep[i] and keep[j]]
    n_atoms = sum(keep)
    c = [mix2(SEED_COLOUR, types[i] + 1) if keep[i] else 0 for i in range(n)]
    for _ in range(n_atoms):
        s = [0] * n
        for i, j, o in kept_bonds:
            s[i] = (s[i] + mix2(c[j], o)) & M
            s[j] = (s[j] + mix2(c[i], o)) & M
        c = [mix2(c[i], s[i]) if keep[i] else 0 for i in range(n)]
    total = sum(mix64(c[i]) for i in range(n) if keep[i]) & M
    key = mix2(mix2(mix2(SEED_KEY, n_atoms), len(kept_bonds)), total)
    return c, key, n_atoms, len(kept_bonds)


def valences_and_pieces(types, bonds, keep=None):
    """Valence per atom over the kept bonds (0 for dropped atoms) and the number of pieces of the kept graph (union-find)."""
    n = len(types)
    keep = [True] * n if keep is None else [bool(k) for k in keep]
    valence, parent = [0] * n, list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j, o in bonds:
        if keep[i] and keep[j]:
            valence[i] += o
            valence[j] += o
            parent[find(i)] = find(j)
    return valence, len({find(i) for i in range(n) if keep[i]})
