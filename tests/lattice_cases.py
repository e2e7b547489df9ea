"""Molecules whose atoms sit on a lattice of dyadic coordinates, so that pairs lie EXACTLY on the distance cut-offs of the
radius graphs (egnn.py:554-596, ``<= 4`` / ``<= 10``), of bond perception (molecule_builder.py:90-98, ``100 * d < T``) and of
the size predictor (linker_size_lightning.py:107, squared distance ``< 6``) - the inputs of tests/test_gpu_cutoff_ties.py -
and the preconditions that keep those tests from passing vacuously (``problems``, asserted by tests/test_cutoff_ties_host.py).

Why no tolerance is needed.  Every coordinate is a small multiple of a power of two (0.5 A for the graphs and the size
predictor, 0.25 A for the bonds; ``|c| <= 64``), so every product and every partial sum of a squared distance is exact in
fp32 in any summation order, with or without fma contraction, and in the ``|a|^2 + |b|^2 - 2ab`` form of the reference's
``cdist``.  A pair is then exactly on a cut-off or at least one lattice step of the squared distance (0.25 A^2) away from it,
and the only thing an implementation can get wrong is the comparison operator.

The values next to a cut-off ("one fp32 step inside / outside") cannot be lattice points.  They use one atom AT THE ORIGIN
and a partner on a coordinate axis at ``nextafter(cut, +-inf)``: the squared distance is ``fl(c * c)`` under every formula.
A pair of such an off-lattice atom with any OTHER atom is not exact; for those pairs ``problems`` asks instead that all four
evaluations (fp64, two fp32 summation orders, the ``cdist`` form) stay ``MARGIN - 2^-10`` away from every cut-off that
applies (the atom is within 2^-20 A of a lattice point and coordinates are below 128 A apart, so its squared distances move
by less than 2^-12 A^2) - nothing is excluded from any comparison.
"""
import contextlib
import functools
import os
import types

import numpy as np
import torch

import test_gpu_parity as P
from helpers import seeded_size_state_dict, seeded_state_dict
from oracle import egnn_oracle, size_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cutoff_ties.npz')
NF = 9
GRAPHS = ('FC-10A-4A', 'FC-4A', '4A')
STEP = 0.5                     # lattice step of the graphs and of the size predictor (A)
BOND_STEP = 0.25               # lattice step of the bond molecules (A)
MARGIN = 0.25                  # A^2: a pair that is not a tie is at least this far from every cut-off that applies to it
OFF_LATTICE_SLACK = 2.0 ** -10
BOND_BAND = 1e-5               # the band of tests/golden/make_golden_bonds.py
POCKET_LAYOUT = dict(batch=2, n_frag=12, n_pocket=40, linker=(4, 9), nf=NF)
# graph -> seed: the first of 901, 1001, ... whose batch meets every precondition (the search still runs and ends at its
# first candidate)
POCKET_SEEDS = {'FC-10A-4A': 901, 'FC-4A': 901, '4A': 901}
POCKET_WEIGHTS = dict(n_layers=2, seed=31)
SIZE_SEED = 41
BOND_SEED = 2024


def f32(v):
    return np.asarray(v, dtype=np.float32)


def next_inside(cut):
    return float(np.nextafter(np.float32(cut), np.float32(0)))


def next_outside(cut):
    return float(np.nextafter(np.float32(cut), np.float32(np.inf)))


def squared_distances(x):
    """``[n, n]`` squared distances of fp32 coordinates ``x [n, 3]`` evaluated four ways: fp64; fp32 ``(xx + yy) + zz``; fp32
    ``xx + (yy + zz)``; fp32 ``|a|^2 + |b|^2 - 2ab`` (the matrix-multiply form of ``torch.cdist``)."""
    x = f32(x)
    d64 = x[:, None].astype(np.float64) - x[None].astype(np.float64)
    exact = (d64 * d64).sum(-1)
    d = x[:, None] - x[None]
    s = d * d
    a = (s[..., 0] + s[..., 1]) + s[..., 2]
    b = s[..., 0] + (s[..., 1] + s[..., 2])
    sq = x * x
    n2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    dot = (x[:, None, 0] * x[None, :, 0] + x[:, None, 1] * x[None, :, 1]) + x[:, None, 2] * x[None, :, 2]
    c = (n2[:, None] + n2[None]) - np.float32(2) * dot
    assert a.dtype == b.dtype == c.dtype == np.float32
    return exact, a, b, c


def exact_pairs(off):
    """``[n, n]`` bool: pairs of two lattice atoms - their squared distance is exact in fp32."""
    return ~off[:, None] & ~off[None]


def one_step_pairs(off, origin):
    """``[n, n]`` bool: the origin atom with an off-lattice axis atom - ``fl(c * c)`` under every fp32 formula."""
    out = np.zeros((len(off), len(off)), dtype=bool)
    if origin is not None:
        out[origin, off] = out[off, origin] = True
    return out


def lattice_problems(tag, x, off, step):
    out = []
    q = x[~off].astype(np.float64) / step
    if not np.array_equal(q, np.round(q)):
        out.append(f'{tag}: a coordinate is no multiple of {step}')
    if np.abs(x).max() > 64:
        out.append(f'{tag}: a coordinate beyond 64 A')
    return out


def exactness_problems(tag, x, off, origin):
    exact, a, b, c = squared_distances(x)
    ok, step = exact_pairs(off), one_step_pairs(off, origin)
    out = []
    for name, v in (('(xx+yy)+zz', a), ('xx+(yy+zz)', b), ('|a|^2+|b|^2-2ab', c)):
        bad = ok & (v.astype(np.float64) != exact)
        if bad.any():
            out.append(f'{tag}: {int(bad.sum())} squared distances differ from fp64 as {name}')
        bad = step & (v != a)
        if bad.any():
            out.append(f'{tag}: {int(bad.sum())} one-step squared distances depend on the formula ({name})')
    return out


# ---- radius graphs ----------------------------------------------------------------------------------------------------------
AXES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def cross_cut(graph_type):
    return 10.0 if graph_type == 'FC-10A-4A' else 4.0


def _plant(graph_type, g, n_frag, n_pocket, n_link):
    """Move atoms of one molecule (integer coordinates ``g`` in lattice steps) onto the ties.  Returns the origin atom and the
    list ``(atom, axis, sign, cut, inside)`` of its axis neighbours."""
    F = list(range(n_frag))
    K = list(range(n_frag, n_frag + n_pocket))
    L = list(range(n_frag + n_pocket, n_frag + n_pocket + n_link))
    v = lambda *c: torch.tensor(c, dtype=g.dtype)                    # noqa: E731
    c4, cx = 8, int(round(cross_cut(graph_type) / STEP))
    # ligand-ligand pairs at 4 A: ties under '4A' (fragment-fragment, linker-linker, fragment-linker), always joined otherwise
    g[F[5]] = g[F[4]] + v(c4, 0, 0)
    g[L[1]] = g[L[0]] + v(0, c4, 0)
    g[L[2]] = g[F[6]] + v(0, 0, c4)
    # the origin atom (a pocket atom) and its six axis neighbours; the neighbours leave the lattice in `lattice_pocket_case`
    origin = K[0]
    g[origin] = 0
    axis = [(K[1], 0, +1, 4.0, True), (K[2], 0, -1, 4.0, False), (K[3], 2, +1, 4.0, True),
            (F[7], 1, +1, cross_cut(graph_type), True), (F[8], 1, -1, cross_cut(graph_type), False),
            (F[9], 2, -1, cross_cut(graph_type), False)]
    for atom, ax, sign, cut, _ in axis:
        g[atom] = 0
        g[atom, ax] = sign * int(round(cut / STEP))
    g[K[4]] = g[K[5]]                                                # two real atoms at one point
    for k, e in enumerate(AXES):                                     # pocket-pocket: a star, all six axis directions
        g[K[7 + k]] = g[K[6]] + c4 * v(*e)
    if cx == c4:
        off_f = [v(c4, 0, 0), v(-c4, 0, 0), v(0, c4, 0), v(0, -c4, 0)]
        off_l = [v(0, 0, c4), v(0, 0, -c4), v(-c4, 0, 0), v(0, c4, 0)]
    else:                                                            # 10 A: (10, 0, 0) and (6, 8, 0) and their permutations
        off_f = [v(20, 0, 0), v(-20, 0, 0), v(0, 12, 16), v(16, 0, -12)]
        off_l = [v(0, 20, 0), v(0, 0, -20), v(12, 16, 0), v(-16, 12, 0)]
    for k in range(4):                                               # ligand-pocket: four on fragment atoms, four on linker atoms
        g[K[13 + k]] = g[F[k]] + off_f[k]
        g[K[17 + k]] = g[L[k]] + off_l[k]
    return origin, axis


def _build_pocket(graph_type, seed):
    inp, z, t = P.pocket_inputs(seed=seed, **POCKET_LAYOUT)
    inp = {k: v.clone() for k, v in inp.items()}
    z = z.clone()
    B, N = z.shape[:2]
    off = torch.zeros(B, N, dtype=torch.bool)
    origins, axes = [], []
    for b in range(B):
        real = inp['node_mask'][b, :, 0] != 0
        n = int(real.sum())
        n_link = int(inp['linker_mask'][b].sum())
        assert bool(real[:n].all()) and n == POCKET_LAYOUT['n_frag'] + POCKET_LAYOUT['n_pocket'] + n_link
        g = torch.round(z[b, :n, :3].double() / STEP).long()
        origin, axis = _plant(graph_type, g, POCKET_LAYOUT['n_frag'], POCKET_LAYOUT['n_pocket'], n_link)
        x = (g.double() * STEP).float()
        for atom, ax, sign, cut, inside in axis:
            x[atom, ax] = sign * (next_inside(cut) if inside else next_outside(cut))
            off[b, atom] = True
        z[b, :n, :3] = x
        origins.append(origin)
        axes.append(axis)
    z[..., :3] *= inp['node_mask']
    inp['x'] = z[..., :3].clone()                                    # the chain starts from the same fragment and pocket atoms
    return types.SimpleNamespace(kind='pocket', graph=graph_type, inp=inp, z=z, t=t, off=off, origins=origins, axes=axes)


def pocket_kinds(case):
    """``(real, fragment, pocket, linker)`` bool ``[B, N]``."""
    inp = case.inp
    real = inp['node_mask'][..., 0] != 0
    pock = (inp['context'][..., -1] != 0) & real
    frag = (inp['context'][..., -2] != 0) & real
    link = (inp['linker_mask'][..., 0] != 0) & real
    return real, frag, pock, link


def pocket_cut2(case, b):
    """``[N, N]`` float64: the squared cut-off that applies to every pair of molecule ``b`` (inf: always joined; nan: never -
    the diagonal and pairs with a padding row)."""
    real, frag, pock, link = (m[b].numpy() for m in pocket_kinds(case))
    lig = frag | link
    n = len(real)
    cut2 = np.full((n, n), np.nan)
    both = real[:, None] & real[None]
    if case.graph == '4A':
        cut2[both] = 16.0
    else:
        cut2[lig[:, None] & lig[None]] = np.inf
        cut2[pock[:, None] & pock[None]] = 16.0
        cut2[(lig[:, None] & pock[None]) | (pock[:, None] & lig[None])] = cross_cut(case.graph) ** 2
    np.fill_diagonal(cut2, np.nan)
    return cut2


def pocket_reference_adjacency(case, edges):
    """The recorded edge index ``[2, E]`` of the reference over the flattened batch as ``[B, N, N]`` bool."""
    B, N = case.z.shape[:2]
    adj = np.zeros((B * N, B * N), dtype=bool)
    adj[edges[0], edges[1]] = True
    out = np.stack([adj[b * N:(b + 1) * N, b * N:(b + 1) * N] for b in range(B)])
    assert out.sum() == adj.sum(), 'an edge between two molecules'
    return out


def pocket_tie_counts(case):
    """Per molecule: ties by kind pair, directions of the pocket-pocket ties, coincident pairs."""
    real, frag, pock, link = (m.numpy() for m in pocket_kinds(case))
    out = []
    for b in range(case.z.shape[0]):
        x = case.z[b, :, :3].numpy()
        exact = squared_distances(x)[0]
        cut2 = pocket_cut2(case, b)
        tie = np.triu(exact == cut2, 1)
        kind = np.where(frag[b], 'F', np.where(pock[b], 'P', np.where(link[b], 'L', '-')))
        counts, dirs, families = {}, set(), set()
        for i, j in zip(*np.nonzero(tie)):
            key = ''.join(sorted(kind[i] + kind[j]))
            counts[key] = counts.get(key, 0) + 1
            delta = x[j] - x[i]
            if key == 'PP' and np.count_nonzero(delta) == 1:
                dirs.add(tuple(np.sign(delta).astype(int)))
            if key in ('FP', 'LP'):
                families.add(np.count_nonzero(delta))
        same = np.triu((exact == 0) & (real[b][:, None] & real[b][None]), 1)
        out.append(dict(counts=counts, directions=dirs, families=families, coincident=int(same.sum())))
    return out


def pocket_problems(case, reference_edges=None):
    out = []
    B, N = case.z.shape[:2]
    if N % 32 == 0 or N <= 32:
        out.append(f'N = {N}: a multiple of 32, or a single row tile')
    ref = None if reference_edges is None else pocket_reference_adjacency(case, reference_edges)
    for b, info in enumerate(pocket_tie_counts(case)):
        tag = f'{case.graph}, molecule {b}'
        x = case.z[b, :, :3].numpy()
        off = case.off[b].numpy()
        out += lattice_problems(tag, x, off, STEP)
        out += exactness_problems(tag, x, off, case.origins[b])
        counts = info['counts']
        if counts.get('PP', 0) < 6 or len(info['directions']) < 6:
            out.append(f'{tag}: {counts.get("PP", 0)} pocket-pocket ties in {len(info["directions"])} axis directions')
        if counts.get('FP', 0) + counts.get('LP', 0) < 6 or counts.get('FP', 0) < 3 or counts.get('LP', 0) < 1:
            out.append(f'{tag}: ligand-pocket ties {counts}')
        if case.graph == 'FC-10A-4A' and not {1, 2} <= info['families']:
            out.append(f'{tag}: the (10, 0, 0) and the (6, 8, 0) family are not both there')
        if case.graph == '4A' and not all(counts.get(k, 0) >= 1 for k in ('FF', 'FL', 'LL', 'FP', 'LP', 'PP')):
            out.append(f'{tag}: not every kind of pair has a tie: {counts}')
        if info['coincident'] < 1:
            out.append(f'{tag}: no two real atoms at one point')
        inside = [a for a in case.axes[b] if a[4]]
        outside = [a for a in case.axes[b] if not a[4]]
        cuts = {a[3] for a in inside} & {a[3] for a in outside}
        wanted = {4.0, 10.0} if case.graph == 'FC-10A-4A' else {4.0}
        if len(inside) < 2 or len(outside) < 2 or len({(a[1], a[2]) for a in case.axes[b]}) < 6 or cuts != wanted:
            out.append(f'{tag}: the axis neighbours of the origin atom do not cover {wanted} inside and outside')
        if np.abs(x[case.origins[b]]).max() != 0:
            out.append(f'{tag}: the origin atom is not at the origin')
        # every pair: tie, or clear of its cut-off; and the decisions agree
        exact, a32, b32, c32 = squared_distances(x)
        cut2 = pocket_cut2(case, b)
        applies = np.isfinite(cut2)
        ok, one_step = exact_pairs(off), one_step_pairs(off, case.origins[b])      # (the one-step pairs: checked below)
        for v in (exact, a32, b32, c32):
            gap = np.abs(v.astype(np.float64) - cut2)
            near = applies & ~one_step & (v != cut2) & (gap < np.where(ok, MARGIN, MARGIN - OFF_LATTICE_SLACK))
            if near.any():
                out.append(f'{tag}: {int(near.sum())} pairs that are no tie within {MARGIN} A^2 of their cut-off')
        want = ~np.isnan(cut2) & (exact <= cut2)
        cut = np.sqrt(cut2)
        decisions = {'fp32 squared': a32 <= cut2, 'fp32 squared, other order': b32 <= cut2, 'fp32 cdist form': c32 <= cut2,
                     'fp32 sqrt': np.sqrt(a32) <= f32(cut), 'fp32 sqrt of the cdist form': np.sqrt(np.maximum(c32, 0)) <= f32(cut)}
        if ref is not None:
            decisions['recorded reference'] = ref[b]
        for name, got in decisions.items():
            got = got & ~np.isnan(cut2)
            if not np.array_equal(got, want):
                out.append(f'{tag}: the {name} decision differs from fp64 on {int((got != want).sum())} pairs')
        # the one-step neighbours are what they claim to be
        for atom, ax, sign, c, is_in in case.axes[b]:
            d2 = a32[case.origins[b], atom]
            if (d2 <= np.float32(c * c)) != is_in or abs(abs(x[atom, ax]) - c) > 1e-6:
                out.append(f'{tag}: axis neighbour {atom} is not one step {"inside" if is_in else "outside"} {c}')
    return out


def _search(build, problems, seed):
    for k in range(100):
        case = build(seed + 100 * k)
        if not problems(case):
            case.seed = seed + 100 * k
            return case
    raise AssertionError('no seed meets the preconditions')


@functools.lru_cache(maxsize=None)
def lattice_pocket_case(graph_type):
    """The pocket batch of ``graph_type``: ``case.inp`` (the sampler inputs, ``x`` on the lattice), ``case.z``, ``case.t``.  Shared:
    read-only."""
    return _search(lambda s: _build_pocket(graph_type, s), pocket_problems, POCKET_SEEDS[graph_type])


def pocket_state_dict(dtype=torch.float32, coord_gain=0.02):
    return seeded_state_dict(NF + 3, 128, POCKET_WEIGHTS['n_layers'], POCKET_WEIGHTS['seed'], coord_gain=coord_gain, dtype=dtype)


def pocket_config(graph_type):
    return egnn_oracle.EGNNConfig(in_node_nf=NF, context_node_nf=2, n_layers=POCKET_WEIGHTS['n_layers'], graph_type=graph_type)


def flipped_pocket_edges(cfg, x, node_mask, batch_mask, linker_mask, fragment_only_mask, pocket_only_mask, which='all'):
    """``egnn_oracle.pocket_edges`` with ``<`` where the reference has ``<=``: the mutants the tests must tell from the truth.
    ``which``: 'all', or one comparison of the FC graphs alone - 'pocket' (pocket-pocket) or 'cross' (ligand-pocket)."""
    nm = node_mask.squeeze(-1).bool()
    base = (batch_mask[:, None] == batch_mask[None, :]) & (nm[:, None] & nm[None, :]) & \
        ~torch.eye(x.size(0), dtype=torch.bool, device=x.device)
    dist = torch.cdist(x, x)
    if cfg.graph_type == '4A':
        adj = base & (dist < 4)
    else:
        lig = (linker_mask.squeeze(-1).bool() | fragment_only_mask.squeeze(-1).bool()) & nm
        poc = pocket_only_mask.squeeze(-1).bool() & nm
        cut = 4 if cfg.graph_type == 'FC-4A' else 10
        near_pocket = (dist < 4) if which in ('all', 'pocket') else (dist <= 4)
        near_cross = (dist < cut) if which in ('all', 'cross') else (dist <= cut)
        cross = ((lig[:, None] & poc[None, :]) | (poc[:, None] & lig[None, :])) & near_cross
        adj = ((lig[:, None] & lig[None, :]) | ((poc[:, None] & poc[None, :]) & near_pocket) | cross) & base
    return torch.where(adj)


@contextlib.contextmanager
def flipped_graph(which='all'):
    true = egnn_oracle.pocket_edges
    egnn_oracle.pocket_edges = functools.partial(flipped_pocket_edges, which=which)
    try:
        yield
    finally:
        egnn_oracle.pocket_edges = true


def pocket_oracle_forward(case, dtype=torch.float64, coord_gain=0.02, inp=None, z=None, t=None):
    inp, z, t = inp or case.inp, case.z if z is None else z, case.t if t is None else t
    return egnn_oracle.dynamics_forward_pockets(pocket_state_dict(dtype, coord_gain), pocket_config(case.graph), t.to(dtype),
                                                z.to(dtype), inp['node_mask'].to(dtype), inp['linker_mask'].to(dtype),
                                                inp['edge_mask'], inp['context'].to(dtype))


def pocket_oracle_grads(case, G, dtype=torch.float64):
    """fp64 autograd of ``sum(out * G)`` through the oracle, by state-dict key."""
    p = {k: v.requires_grad_(True) for k, v in pocket_state_dict(dtype).items()}
    inp = case.inp
    out = egnn_oracle.dynamics_forward_pockets(p, pocket_config(case.graph), case.t.to(dtype), case.z.to(dtype),
                                               inp['node_mask'].to(dtype), inp['linker_mask'].to(dtype), inp['edge_mask'],
                                               inp['context'].to(dtype))
    (out * G.to(dtype)).sum().backward()
    return {k: v.grad for k, v in p.items()}


def cotangent(case, seed=7):
    return torch.randn(case.z.shape, generator=torch.Generator().manual_seed(seed))


def pocket_oracle_chain(case, T, noise_seed, coord_gain, keep_frames=2):
    from oracle import edm_oracle
    inp = case.inp
    B, N = inp['x'].shape[:2]
    bank = edm_oracle.NoiseBank.generate(T, B, N, 3, NF, seed=noise_seed)
    orc = edm_oracle.EDMOracle(edm_oracle.make_dynamics_oracle(pocket_state_dict(coord_gain=coord_gain), pocket_config(case.graph)),
                               in_node_nf=NF, timesteps=500)
    orc.T = T
    want = orc.sample_chain(inp['x'], inp['h'], inp['node_mask'], inp['fragment_mask'], inp['linker_mask'], inp['edge_mask'],
                            inp['context'], bank, keep_frames=keep_frames)
    return want, bank


# ---- bonds --------------------------------------------------------------------------------------------------------------------
C, O, N_, F_, S_ = 0, 1, 2, 3, 4                                     # const.IDX2ATOM / GEOM_IDX2ATOM start alike
BOND_WIDTH = 64
# steps of the long chains, A: lattice vectors of bond length, the two tie lengths among them
CHAIN_STEPS = ((1.25, 0, 0), (0.75, 1.0, 0), (1.5, 0, 0), (1.0, 1.0, 0.5), (1.0, 1.0, 0.25), (1.25, 0.5, 0), (1.0, 0.75, 0.5))


def _small_bond_molecules():
    """``(name, [(element, (x, y, z))], off-lattice atoms, origin atom)``: the constructions ``bond_problems`` counts."""
    eps_c, eps_n = next_inside(1.25), next_inside(1.5)

    def shifted(atoms, base, sign=1.0):
        return [(e, tuple(sign * c + o for c, o in zip(p, base))) for e, p in atoms]
    ties = [(C, (0, 0, 0)), (O, (1.25, 0, 0)),                      # C-O on an axis at 1.25 A: single, not double
            (N_, (2.75, 0, 0)),                                     # O-N on an axis at 1.5 A: no bond
            (C, (2.75, 1.25, 0)),
            (O, (3.5, 2.25, 0)),                                    # C-O as (0.75, 1, 0)
            (N_, (4.5, 3.25, 0.5))]                                 # O-N as (1, 1, 0.5)
    split = [(C, (0, 0, 0)), (C, (1.5, 0, 0)), (O, (2.75, 0, 0)), (N_, (2.75, 1.5, 0)), (C, (2.75, 2.75, 0))]
    inside = [(O, (0, 0, 0)), (C, (eps_c, 0, 0)), (N_, (0, eps_n, 0)), (C, (0, 0, -eps_c)), (N_, (-eps_n, 0, 0)),
              (C, (0, -eps_c, 0)), (N_, (0, 0, eps_n))]
    same = [(C, (0, 0, 0)), (C, (0, 0, 0)), (O, (1.25, 0, 0)), (N_, (1.25, 1.5, 0)), (O, (1.25, 1.5, 0))]
    return [('ties, C before O', shifted(ties, (2.0, -1.25, 0.5)), [], None),
            ('ties, O before C', shifted(ties, (-1.0, 0.75, 2.0), -1.0)[::-1], [], None),
            ('split', shifted(split, (0.5, 0.5, -1.0)), [], None),
            ('split, reversed', shifted(split, (-0.25, 1.0, 0.0), -1.0)[::-1], [], None),
            ('one step inside, O first', inside, list(range(1, 7)), 0),
            ('one step inside, O last', inside[::-1], list(range(0, 6)), 6),
            ('coincident', shifted(same, (1.0, 1.0, 1.0)), [], None)]


def _chain_molecule(rng, n, n_types):
    """A self-avoiding walk on the 0.25 A lattice with steps of bond length; C, O and N make up most of it."""
    weights = np.array([4, 3, 3] + [0.5] * (n_types - 3))
    pos = [np.zeros(3)]
    while len(pos) < n:
        parent = pos[-1] if rng.random() < 0.8 else pos[rng.integers(0, len(pos))]
        step = np.array(CHAIN_STEPS[rng.integers(0, len(CHAIN_STEPS))])
        cand = parent + rng.permutation(step) * rng.choice([-1.0, 1.0], size=3)
        if min(np.linalg.norm(cand - p) for p in pos) >= 1.0:
            pos.append(cand)
    types_ = rng.choice(n_types, size=n, p=weights / weights.sum())
    return [(int(e), tuple(p)) for e, p in zip(types_, pos)]


@functools.lru_cache(maxsize=None)
def lattice_bond_molecules(is_geom):
    """One batch ``one_hot [B, 64, nf]``, ``x``, ``mask [B, 64, 1]`` of the bond molecules of one vocabulary, real rows scattered
    between masked junk rows that hold lattice points too - the first junk row of every molecule an oxygen exactly 1.25 A from
    the molecule's first carbon.  ``mols``: the molecules alone, in row order (what the reference is run on)."""
    from difflinker_amd import const
    nf = const.GEOM_NUMBER_OF_ATOM_TYPES if is_geom else const.NUMBER_OF_ATOM_TYPES
    rng = np.random.default_rng(BOND_SEED + int(is_geom))
    specs = _small_bond_molecules()
    for n in (24, 33, 47, 60):
        specs.append((f'chain of {n}', _chain_molecule(rng, n, nf), [], None))
    B = len(specs)
    one_hot = np.zeros((B, BOND_WIDTH, nf), np.float32)
    x = np.zeros((B, BOND_WIDTH, 3), np.float32)
    mask = np.zeros((B, BOND_WIDTH, 1), np.float32)
    off = np.zeros((B, BOND_WIDTH), bool)
    mols, origins = [], []
    for b, (name, atoms, off_atoms, origin) in enumerate(specs):
        n = len(atoms)
        rows = np.sort(rng.choice(BOND_WIDTH, size=n, replace=False)) if n < BOND_WIDTH else np.arange(n)
        types_ = np.array([e for e, _ in atoms])
        pos = f32([p for _, p in atoms])
        mask[b, rows] = 1
        x[b, rows] = pos
        one_hot[b, rows, types_] = 1
        off[b, rows[off_atoms]] = True
        origins.append(None if origin is None else int(rows[origin]))
        junk = np.setdiff1d(np.arange(BOND_WIDTH), rows)
        x[b, junk] = pos[rng.integers(0, n, size=len(junk))] + \
            BOND_STEP * rng.integers(-6, 7, size=(len(junk), 3)).astype(np.float32)
        one_hot[b, junk, rng.integers(0, nf, size=len(junk))] = 1
        carbon = np.nonzero(types_ == C)[0]
        if len(carbon) and len(junk) and not off[b, rows[carbon[0]]]:
            x[b, junk[0]] = pos[carbon[0]] + f32([0, 1.25, 0])
            one_hot[b, junk[0]] = 0
            one_hot[b, junk[0], O] = 1
        mols.append((name, types_, pos))
    return types.SimpleNamespace(kind='bonds', is_geom=is_geom, one_hot=torch.from_numpy(one_hot), x=torch.from_numpy(x),
                                 mask=torch.from_numpy(mask), off=off, origins=origins, mols=mols)


def bond_order_fp64(table, a, b, d):
    """``get_bond_order`` (molecule_builder.py:78-102) for element indices and a distance in A; ``table``:
    ``const.bond_threshold_table`` as a nested list (a missing order is a negative bound, which no distance is below)."""
    d = 100.0 * d
    lo, hi = min(a, b), max(a, b)                                    # the reference looks the pair up lower index first
    t = table[lo][hi]
    if not d < t[0]:
        return 0
    if not d < t[1]:
        return 1
    return 3 if d < t[2] else 2


def bond_order_flipped(table, a, b, d):
    """The mutant: ``<=`` where the reference has ``<``."""
    d = 100.0 * d
    t = table[min(a, b)][max(a, b)]
    if not (t[0] > 0 and d <= t[0]):
        return 0
    if not (t[1] > 0 and d <= t[1]):
        return 1
    return 3 if (t[2] > 0 and d <= t[2]) else 2


def bond_matrix(is_geom, types_, pos, order=bond_order_fp64):
    """``E`` of ``build_xae_molecule`` (lower triangle) from fp64 distances of the fp32 coordinates."""
    from difflinker_amd import const
    table = const.bond_threshold_table(is_geom).double().tolist()
    p = np.asarray(pos, dtype=np.float64)
    n = len(types_)
    E = np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(i):
            E[i, j] = order(table, int(types_[i]), int(types_[j]), float(np.sqrt(((p[i] - p[j]) ** 2).sum())))
    return E


def pieces(E):
    n = len(E)
    label = list(range(n))

    def find(a):
        while label[a] != a:
            a = label[a]
        return a
    for i, j in zip(*np.nonzero(E)):
        ri, rj = find(i), find(j)
        label[max(ri, rj)] = min(ri, rj)
    return len({find(a) for a in range(n)})


def bond_problems(case, reference_E=None):
    from difflinker_amd import const
    table = const.bond_threshold_table(case.is_geom).numpy().astype(np.float64)
    out, seen = [], dict(co_axis=0, co_diag=0, on_axis=0, on_diag=0, inside2=0, inside1=0, o_first=0, o_last=0, same=0)
    for b, (name, types_, pos) in enumerate(case.mols):
        tag = f'{"GEOM" if case.is_geom else "ZINC"} {name}'
        rows = np.nonzero(case.mask[b, :, 0].numpy())[0]
        off = case.off[b][rows]
        origin = None if case.origins[b] is None else int(np.nonzero(rows == case.origins[b])[0][0])
        if not np.array_equal(case.x[b].numpy()[rows], pos):
            out.append(f'{tag}: the batch does not hold the molecule')
        if len(types_) > 24 and not 30 <= len(types_) <= 60:
            out.append(f'{tag}: {len(types_)} atoms')
        out += lattice_problems(tag, pos, off, BOND_STEP)
        out += exactness_problems(tag, pos, off, origin)
        exact, a32, b32, c32 = squared_distances(pos)
        E64 = bond_matrix(case.is_geom, types_, pos)
        n = len(types_)
        for i in range(n):
            for j in range(i):
                thr = [t for t in table[types_[i], types_[j]] if t > 0]
                d = 100.0 * np.sqrt(exact[i, j])
                tie = [t for t in thr if d == t]
                one_step = origin in (i, j) and (off[i] or off[j])
                if not one_step and any(abs(d / t - 1) < BOND_BAND for t in thr if t not in tie):
                    out.append(f'{tag}: pair {i}, {j} within a relative {BOND_BAND} of a threshold it is not on')
                # the fp32 decisions: direct, and through the matrix-multiply form of cdist
                for name32, v in (('direct', a32), ('other order', b32), ('cdist form', c32)):
                    d32 = np.float32(100) * np.sqrt(np.maximum(v[i, j], np.float32(0)))
                    o32 = 0
                    for k, t in enumerate(table[types_[i], types_[j]]):
                        if t > 0 and d32 < np.float32(t) and o32 == k:
                            o32 = k + 1
                    if o32 != E64[i, j]:
                        out.append(f'{tag}: pair {i}, {j}: fp32 {name32} order {o32}, fp64 {E64[i, j]}')
                pair = {int(types_[i]), int(types_[j])}
                delta = pos[i] - pos[j]
                axis = np.count_nonzero(delta) == 1
                if tie and pair == {C, O} and d == 125.0:
                    seen['co_axis' if axis else 'co_diag'] += 1
                    seen['o_first' if types_[j] == O else 'o_last'] += 1
                    if E64[i, j] != 1:
                        out.append(f'{tag}: a C-O pair at 1.25 A with order {E64[i, j]}')
                if tie and pair == {O, N_} and d == 150.0:
                    seen['on_axis' if axis else 'on_diag'] += 1
                    if E64[i, j] != 0:
                        out.append(f'{tag}: an O-N pair at 1.5 A with order {E64[i, j]}')
                if origin in (i, j) and (off[i] or off[j]):
                    seen['inside2'] += pair == {C, O} and E64[i, j] == 2
                    seen['inside1'] += pair == {O, N_} and E64[i, j] == 1
                if exact[i, j] == 0:
                    seen['same'] += 1
                    if E64[i, j] != sum(t > 0 for t in table[types_[i], types_[j]]):
                        out.append(f'{tag}: coincident atoms do not take the highest order of their pair')
        if name.startswith('split'):
            flipped = bond_matrix(case.is_geom, types_, pos, bond_order_flipped)
            if pieces(E64) != 2 or pieces(flipped) != 1:
                out.append(f'{tag}: {pieces(E64)} pieces, {pieces(flipped)} with the O-N pair bonded')
        if reference_E is not None and not np.array_equal(reference_E[b][:n, :n], E64):
            out.append(f'{tag}: the recorded reference matrix differs from fp64 on {int((reference_E[b][:n, :n] != E64).sum())} pairs')
    if min(seen.values()) < 1 or seen['inside2'] < 2 or seen['inside1'] < 2:
        out.append(f'a construction is missing: {seen}')
    junk_hits = 0
    for b in range(len(case.mols)):
        m = case.mask[b, :, 0].numpy() != 0
        xs, ts = case.x[b].numpy().astype(np.float64), case.one_hot[b].numpy().argmax(1)
        d = np.sqrt(((xs[~m][:, None] - xs[m][None]) ** 2).sum(-1))
        junk_hits += int(((d == 1.25) & (ts[~m][:, None] == O) & (ts[m][None] == C)).sum())
    if junk_hits < 1:
        out.append('no masked oxygen exactly 1.25 A from a real carbon')
    return out


# ---- size predictor -------------------------------------------------------------------------------------------------------------
SIZE_IN_NF, SIZE_OUT_NF = 8, 10
SIZE_MOLS = ([16, 64, 30], [3, 0, 6])                                # atoms, of which linker atoms (dropped by the fragment mask)
# lattice steps (A): squared lengths 3, 6 (the tie), 3.5, 5.25, 6.25, 5.5
SIZE_STEPS = ((1, 1, 1), (2, 1, 1), (1.5, 1, 0.5), (2, 1, 0.5), (2, 1.5, 0), (1.5, 1.5, 1))
SIZE_MODELS = {'plain': (3, False), 'bn': (2, True)}                # tag -> layers, BatchNorm (the models of size_gnn.npz)


@functools.lru_cache(maxsize=None)
def lattice_size_case():
    """A ``collate_with_fragment_edges`` batch whose fragments are walks on the 0.5 A lattice, two steps of three a
    permutation of (2, 1, 1) - squared length 6 exactly; and, for the precomputed-distances entry, the squared distances
    of the batch with the entries of molecule 0's pairs (0, 1) and (1, 2) replaced by ``nextafter(6, -+inf)``."""
    from difflinker_amd.datasets import collate_with_fragment_edges
    rng = np.random.default_rng(SIZE_SEED)
    g = torch.Generator().manual_seed(SIZE_SEED)
    mols = []
    for n, nl in zip(*SIZE_MOLS):
        pos = [np.zeros(3)]
        while len(pos) < n:
            step = np.array(SIZE_STEPS[1] if len(pos) % 3 != 0 else SIZE_STEPS[rng.integers(0, len(SIZE_STEPS))], dtype=float)
            cand = pos[-1] + rng.permutation(step) * rng.choice([-1.0, 1.0], size=3)
            if min(np.linalg.norm(cand - p) for p in pos) >= 1.0:
                pos.append(cand)
        pos = torch.tensor(np.array(pos), dtype=torch.float32)
        pos = pos - torch.round(pos.mean(0) / STEP) * STEP          # near the origin, still on the lattice
        frag = torch.zeros(n)
        frag[:n - nl] = 1
        kinds = torch.randint(0, SIZE_IN_NF, (n,), generator=g)
        mols.append({'positions': pos, 'one_hot': torch.nn.functional.one_hot(kinds, SIZE_IN_NF).float(), 'anchors': torch.zeros(n),
                     'fragment_mask': frag, 'linker_mask': 1 - frag, 'num_atoms': n, 'uuid': 0, 'name': 'm'})
    data = collate_with_fragment_edges(mols)
    B, N = data['positions'].shape[:2]
    x = data['positions'] * data['fragment_mask']
    distances = ((x[:, :, None] - x[:, None]) ** 2).sum(-1)
    lo, hi = np.nextafter(np.float32(6), np.float32(0)), np.nextafter(np.float32(6), np.float32(np.inf))
    for (i, j), v in (((0, 1), lo), ((1, 0), lo), ((1, 2), hi), ((2, 1), hi)):
        distances[0, i, j] = float(v)
    return types.SimpleNamespace(kind='size', data=data, distances=distances, neighbours=(float(lo), float(hi)))


def size_state_dict(tag, dtype=torch.float32):
    L, bn = SIZE_MODELS[tag]
    sd = seeded_size_state_dict(SIZE_IN_NF, 128, SIZE_OUT_NF, L, seed=500 + L, batch_norm=bn, prefix='gnn.')
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def size_logits(case, tag, dtype=torch.float64, keep=lambda d: d < 6, distances=None):
    """``size_oracle.size_classifier_logits`` with the filter as a parameter and, optionally, given squared distances
    ``[B, N, N]`` (linker_size_lightning.py:104-110)."""
    L, bn = SIZE_MODELS[tag]
    d = case.data
    bs, n = d['positions'].shape[:2]
    fm = d['fragment_mask'].to(dtype)
    h = (d['one_hot'].to(dtype) * fm).reshape(bs * n, -1)
    row, col = egnn_oracle.fc_edges(n, bs)
    if distances is None:
        dist, _ = egnn_oracle.coord2diff((d['positions'].to(dtype) * fm).reshape(bs * n, -1), row, col)
    else:
        dist = distances.to(dtype).reshape(-1, 1)
    dmask = (d['edge_mask'].reshape(-1, 1).bool() & keep(dist)).to(dtype)
    out = size_oracle.size_gnn_forward(size_state_dict(tag, dtype), h, row, col, dist, fm.reshape(bs * n, 1), dmask, L, bn, 'gnn.')
    return out.view(bs, n, -1).mean(1)


def size_problems(case):
    out = []
    d = case.data
    frag = d['fragment_mask'][..., 0].numpy() != 0
    for b in range(d['positions'].shape[0]):
        tag = f'size molecule {b}'
        x = (d['positions'][b] * d['fragment_mask'][b]).numpy()
        if frag[b].sum() > 64:
            out.append(f'{tag}: {int(frag[b].sum())} fragment atoms')
        off = np.zeros(len(x), bool)
        out += lattice_problems(tag, x, off, STEP)
        out += exactness_problems(tag, x, off, None)
        exact = squared_distances(x)[0]
        pair = np.triu(frag[b][:, None] & frag[b][None], 1)
        ties = int((pair & (exact == 6)).sum())
        if ties < 8:
            out.append(f'{tag}: {ties} pairs at a squared distance of 6')
        near = pair & (exact != 6) & (np.abs(exact - 6) < MARGIN)
        if near.any():
            out.append(f'{tag}: {int(near.sum())} pairs that are no tie within {MARGIN} of 6')
    lo, hi = case.neighbours
    if not (np.float32(lo) < np.float32(6) < np.float32(hi)) or float(case.distances[0, 0, 1]) != lo or \
            float(case.distances[0, 1, 2]) != hi:
        out.append('the given distances do not hold the two neighbours of 6')
    return out


def size_tie_counts(case):
    d = case.data
    frag = d['fragment_mask'][..., 0].numpy() != 0
    out = []
    for b in range(len(frag)):
        exact = squared_distances((d['positions'][b] * d['fragment_mask'][b]).numpy())[0]
        out.append(int((np.triu(frag[b][:, None] & frag[b][None], 1) & (exact == 6)).sum()))
    return out


# ---- the fixture and the common entry -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/cutoff_ties.npz (tests/golden/make_golden_ties.py: the unmodified reference on the inputs above)."""
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def problems(case, with_reference=True):
    """The preconditions ``case`` misses, as a list of sentences (empty: all hold).  ``with_reference``: compare the decisions
    with the ones recorded from the reference too (the fixture must exist and hold the same inputs)."""
    ref = fixture() if with_reference else None
    if case.kind == 'pocket':
        edges = None
        if ref is not None:
            if not np.array_equal(ref[f'pocket.{case.graph}.xh'], case.z.numpy()):
                return [f'{case.graph}: the fixture was recorded on other inputs']
            edges = ref[f'pocket.{case.graph}.edges']
        return pocket_problems(case, edges)
    if case.kind == 'bonds':
        tag = 'geom' if case.is_geom else 'zinc'
        if ref is not None and not np.array_equal(ref[f'bonds.{tag}.x'], case.x.numpy()):
            return [f'bonds {tag}: the fixture was recorded on other inputs']
        return bond_problems(case, None if ref is None else ref[f'bonds.{tag}.E'])
    if ref is not None and not np.array_equal(ref['size.positions'], case.data['positions'].numpy()):
        return ['size: the fixture was recorded on other inputs']
    return size_problems(case)


# ---- coincident atoms on the fully-connected graph -----------------------------------------------------------------------------
FC_NF = 8
FC_WEIGHTS = dict(n_layers=2, seed=45)
FC_COINCIDENT = {'ragged': ([12, 7], [4, 2], 821), 'two_atoms': ([2], [1], 822)}


@functools.lru_cache(maxsize=None)
def fc_coincident_case(name):
    """``(inp, z, t)`` of tests/test_gpu_parity.py::ragged_inputs with atoms moved onto each other: 'ragged' - in molecule 0
    a linker atom onto a fragment atom, in molecule 1 two fragment atoms; 'two_atoms' - a molecule that is one point.  The
    reference's ``sqrt(r + 1e-8)`` keeps the forward and its gradient finite there."""
    sizes, linkers, seed = FC_COINCIDENT[name]
    # (the two-atom molecule keeps the padded width of the other case: the width itself is not what is under test here)
    inp, z, t = P.ragged_inputs(sizes, linkers, FC_NF, seed=seed, n_pad=None if name == 'ragged' else 12)
    z = z.clone()
    if name == 'ragged':
        z[0, 9, :3] = z[0, 2, :3]
        z[1, 3, :3] = z[1, 0, :3]
    else:
        z[0, 1, :3] = z[0, 0, :3]
    return inp, z, t


def fc_oracle(name, G=None, dtype=torch.float64):
    """The oracle's forward on a coincident case and, with a cotangent ``G``, the gradient of ``sum(out * G)`` by key."""
    inp, z, t = fc_coincident_case(name)
    cfg = egnn_oracle.EGNNConfig(in_node_nf=FC_NF, context_node_nf=1, n_layers=FC_WEIGHTS['n_layers'])
    p = seeded_state_dict(FC_NF + 2, 128, FC_WEIGHTS['n_layers'], FC_WEIGHTS['seed'], dtype=dtype)
    if G is not None:
        p = {k: v.requires_grad_(True) for k, v in p.items()}
    out = egnn_oracle.dynamics_forward(p, cfg, t.to(dtype), z.to(dtype), inp['node_mask'].to(dtype), inp['linker_mask'].to(dtype),
                                       inp['edge_mask'].to(dtype), inp['context'].to(dtype))
    if G is None:
        return out
    (out * G.to(dtype)).sum().backward()
    return out.detach(), {k: v.grad for k, v in p.items()}
