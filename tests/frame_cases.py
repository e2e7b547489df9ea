"""Frame and numbering independence of the 3D analysis kernels: the transforms, the cases, the ``undo`` of every result and the
clearance condition of ``tests/test_frames_host.py`` (the restatements, here) and ``tests/test_gpu_frames.py`` (the kernels).
Host only: numpy and the ``*_ref.py`` restatements.

A sample sits in an arbitrary PDB frame, 50 to 300 A from the origin, with its atoms in an arbitrary order.  The same molecule
in another frame, mirrored, or renumbered must get the same answer.  Nothing here compares a kernel with its restatement:
every check compares ONE implementation with ITSELF on two presentations of one molecule, so it also sees what a kernel and
its restatement share (a cross product with two components swapped, a plane fit that favours an axis, a row index that leaks
into a result).

TRANSFORMS (``TRANSFORMS``; ``y = R x + t``, then a renumbering)
  perm_*     the 24 proper signed axis permutations.  Exact: the fp32 input IS the transformed molecule.
  mirror_*   the 24 improper ones (mirror images), for the entry points whose rule has no handedness (all but
             ``dl_add_hydrogens`` in part, see ``ENTRY_POINTS``; ``dl_best_rmsd`` gets them on both molecules at once).
  rot_*      three seeded random rotations: QR of a Gaussian matrix in fp64, determinant fixed to +1, applied in fp64, the
             result rounded to fp32 once (by the packing).
  shift_*    translations by (0, 0, 0), by a vector of 100 A and by one of 300 A.
  renumber_* a seeded permutation of the real atoms together with a new scatter of the real rows among the padding rows.  The
             bond list keeps its entry order with its indices renamed; masks and ``atom_planar`` go with the atoms,
             ``bond_aromatic`` with the entries; protein / target atoms are permuted independently.

BARS for continuous outputs
  signed permutations, renumberings   ``ULPS`` = 4 ulp of the output's dtype at the largest magnitude of that output in the
                                      molecule: the input is exact and only the order of a three-term sum changes.  Where
                                      the restatement itself needs more, ``PERM_BAR`` holds twice its measured deviation.
  rotations, translations             ``GEOMETRIC`` = 32 x the input rounding (half an fp32 ulp) at the case's largest
                                      coordinate: a Lipschitz constant of order one x 3 coordinates x 2 atoms, a factor 5 to
                                      spare.  Squared outputs (``min_dist2``, ``best_d2``) are compared as distances.
  dl_relax_molecules                  4 x the deviation of the fp64 restatement, measured (``RELAX_DEVIATION``), under every
                                      transform: the minimiser branches on the sign of the power, and its sensitivity to
                                      an input change of 1e-5 A is not derivable.

CLEARANCE.  A discrete result can only be required to stay the same when no decision of the rule sits within input rounding
of its threshold.  ``clearance(entry, inputs)`` lists every decision quantity of the rule, in fp64, as a distance in A (or its
equivalent for a cosine) from its threshold; each must be at least ``MARGIN`` = 1e-3 A: input rounding at 300 A is 2^-16 A =
1.5e-5 A per coordinate, fp32 pair arithmetic adds the same order, and 1e-3 leaves a factor of more than 30.

THE CAP (what keeps this suite from hiding failures)
  * No case is dropped for a transform: a case clears under ALL of its transforms, or its seed is replaced (the first of
    seed, seed + 100, ... that clears; the seeds found are fixed in every entry point's ``SEEDS`` and ``fixed_case`` holds
    them to that).  The random molecules of the bond-list entry points are drawn one by one from their seed and a molecule
    with a decision within 2 x ``MARGIN`` is not taken, as ``hydrogens_ref.random_molecules`` draws them; the case as a whole
    is then held to ``MARGIN`` under every transform by ``test_frames_host`` like every other.
  * Where the header itself says a choice is arbitrary in the frame, the entry point and the header's sentence are listed in
    ``FRAME_DEPENDENT_BY_RULE``; for the cases named there only the frame-free content is compared (counts, parents, X-H
    lengths, H-X-H and H-X-neighbour angles).
  * At most one case in three per entry point falls under that table, and every entry point keeps a case compared in full.
"""
import itertools
import math

import numpy as np

import aromatic_ref as ar
import clash_ref
import hydrogens_ref as hr
import interaction_ref as ir
import pharmacophore_ref as ph
import pocket_ref
import pose_checks_ref as pr
import relax_ref as rr
import rmsd_ref
import shape_ref

MARGIN = 1e-3                  # A: every decision clears its threshold by this much
COS_MARGIN = 2e-3              # the same for a cosine: arms of 0.8 A and more turn by at most 1e-3 / 0.8 rad
ULPS = 4
GEOMETRIC = 32
MAX_B, MAX_ATOMS = 16, 40

# ---- measured deviations of the restatements (tests/test_frames_host.py::test_restatement_deviations_are_those_written_down
# prints them and holds these constants to them).  The GPU bars are multiples of these: the kernels compute in the
# restatements' precision on the same rounded inputs, so anything beyond a small factor is not input rounding.
# dl_relax_molecules, fp64 restatement ``relax_ref.relax``: the largest deviation of every continuous output over all cases and
# transforms of ``ENTRY_POINTS['dl_relax_molecules']`` at ``steps`` 0, 1 and 40 - x_out of the moved rows after the inverse
# motion in A; energy, f_max and moved2 relative to max(1, |value|).  Measured 2026-10-21; the case and transform behind each:
RELAX_DEVIATION = {
    0: dict(x=7.6e-6,          # case 'random', shift_300: the rounding of the input itself, x_out = x
            energy=1.1e-4,     # 'hand', shift_300
            f_max=0.0, moved2=0.0),
    1: dict(x=1.4e-5,          # 'axes', shift_300
            energy=1.1e-4,     # 'hand', shift_300
            f_max=1.2e-4,      # 'hand', shift_300
            moved2=7.6e-8),    # 'axes', shift_300
    40: dict(x=7.7e-4,         # 'random', shift_300
             energy=5.5e-3,    # 'random', shift_300
             f_max=4.9e-3,     # 'random', shift_300
             moved2=2.1e-5),   # 'axes', shift_300
}
RELAX_BAR_FACTOR = 4           # the GPU bar is this multiple.  It was a supposition until the kernel had been run: on an MI355X
#                                its deviations are the restatement's to three digits (7.66e-4 A and 5.44e-3 at 40 steps).
# entry point -> output -> bar under signed permutations and renumberings where 4 ulp do not do: twice the restatement's own
# deviation, with the case and the transform that gave it.  None is needed: the largest deviation of a restatement there is
# 4.4e-16 A (dl_add_hydrogens h_x, case 'random'), below 4 ulp of a coordinate of 3 A.
PERM_BAR = {}

FRAME_DEPENDENT_BY_RULE = {
    'dl_add_hydrogens': {
        'cases': ('axes',),
        'header': ('perp(u): m is the axis with the smallest |u_m| (the lowest m of equal ones), v = e_m - u_m * u',
                   'T4, d = 0   g = 1 / sqrt(3); the first h of (g, g, g), (g, -g, -g), (-g, g, -g), (-g, -g, g).'),
        'compared': 'n_h, h_count, parents, X-H lengths, H-X-H and H-X-neighbour angles',
        # two more choices of the rule are the frame's hand or the numbering, by these lines of the header; they are made per
        # SITE (``Hydrogens.site_kinds``), in every case, and ``test_hydrogen_cases_cover_every_kind_of_site`` counts them: a
        # third or more of the parents of every case are compared in full under every transform (17 of 35 in 'random'), a
        # 'numbered' one (14 of 35) everywhere but under the two renumberings
        'sites': {
            'handed': {'header': ('n = c / |c| when c . c > EPS', 'e2 = u1 x e1.', 'w = (u2 - u1) x (u3 - u1)',
                                  'the first h of them.'),
                       'compared': 'under a mirror or an odd renumbering of the neighbours: in full, against the mirror image of '
                                   'the other free site; otherwise in full'},
            'numbered': {'header': ('r the smallest-numbered neighbour of k other than a.',),
                         'compared': 'under a renumbering: the frame-free content; otherwise in full'},
        },
    },
}


# ---- transforms ----------------------------------------------------------------------------------------------------------------
class Transform:
    def __init__(self, name, kind, R=None, t=None, seed=None):
        self.name, self.kind, self.seed = name, kind, seed
        self.R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
        self.t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64)
        self.exact = kind in ('perm', 'mirror', 'renumber', 'identity') or (kind == 'shift' and not self.t.any())
        self.proper = np.linalg.det(self.R) > 0

    def __repr__(self):
        return self.name

    def apply(self, points):
        """``R x + t`` in fp64 of ``points [..., 3]``; the caller rounds to fp32 once."""
        return np.asarray(points, dtype=np.float64) @ self.R.T + self.t

    def undo(self, points):
        return (np.asarray(points, dtype=np.float64) - self.t) @ self.R

    def sigma(self, n, b, salt=0):
        """The renumbering of molecule ``b``'s ``n`` atoms: old number -> new number (the identity for other transforms)."""
        if self.kind != 'renumber':
            return np.arange(n)
        return np.random.default_rng([self.seed, b, salt]).permutation(n)


def signed_permutations():
    out = []
    for axes in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3))
            for row, (a, s) in enumerate(zip(axes, signs)):
                R[row, a] = s
            name = ''.join('xyz'[a] for a in axes) + ''.join('+' if s > 0 else '-' for s in signs)
            det = round(np.linalg.det(R))
            out.append(Transform(('perm_' if det > 0 else 'mirror_') + name, 'perm' if det > 0 else 'mirror', R))
    return out


def rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


IDENTITY = Transform('identity', 'identity')
PERMS = [t for t in signed_permutations() if t.kind == 'perm']
MIRRORS = [t for t in signed_permutations() if t.kind == 'mirror']
ROTATIONS = [Transform(f'rot_{seed}', 'rot', rotation(seed)) for seed in (11, 12, 13)]
SHIFTS = [Transform('shift_0', 'shift', t=(0.0, 0.0, 0.0)), Transform('shift_100', 'shift', t=(61.3, -52.7, 58.9)),
          Transform('shift_300', 'shift', t=(-171.9, 183.4, 163.7))]
RENUMBERINGS = [Transform(f'renumber_{seed}', 'renumber', seed=seed) for seed in (5, 6)]
LATTICE_SHIFTS = [Transform('lattice_0', 'shift', t=(0.0, 0.0, 0.0)), Transform('lattice_a', 'shift', t=(8.0, -16.0, 32.5)),
                  Transform('lattice_b', 'shift', t=(-100.5, 57.0, 21.5))]
for _t in LATTICE_SHIFTS:
    _t.exact = True
ALL = PERMS + MIRRORS + ROTATIONS + SHIFTS + RENUMBERINGS
TRANSFORMS = {t.name: t for t in ALL + LATTICE_SHIFTS}


def f32(points):
    """fp32 values as float64: the coordinates a kernel reads."""
    return np.asarray(points, dtype=np.float32).astype(np.float64)


def input_rounding(*arrays):
    """Half an fp32 ulp at the largest finite coordinate of the arrays, in A."""
    top = max([float(np.abs(a[np.isfinite(a)]).max()) for a in arrays if np.isfinite(a).any()] + [1.0])
    return float(np.spacing(np.float32(top))) / 2


def ulp(values, dtype):
    top = float(np.abs(np.asarray(values, dtype=np.float64)).max(initial=0.0))
    return float(np.spacing(np.asarray(max(top, 1e-30), dtype=dtype)))


def bar(T, dtype, values, *inputs, entry=None, output=None):
    """The bar of a continuous output of ``dtype`` whose values are ``values``, for transform ``T`` of ``inputs``."""
    if T.exact:
        return max(ULPS * ulp(values, dtype), PERM_BAR.get(entry, {}).get(output, 0.0))
    return GEOMETRIC * input_rounding(*inputs)


# ---- molecules with a bond list -----------------------------------------------------------------------------------------------
def molecule_of(types, points, entries=(), planar=(), marked=(), dropped=(), aromatic=()):
    """A molecule dict of the restatements: ``points`` are fp32 values, so a signed permutation of them is exact."""
    return dict(types=[int(t) for t in types], points=f32(np.asarray(points, dtype=np.float64).reshape(len(types), 3)),
                entries=[tuple(int(v) for v in e) for e in entries], planar=sorted(int(k) for k in planar),
                marked=sorted(int(k) for k in marked), dropped=sorted(int(k) for k in dropped),
                aromatic=sorted(int(e) for e in aromatic))


def moved(m, T, b):
    """Molecule ``b`` of a case under ``T``: the points moved (fp64; the packing rounds once), the atoms renumbered by
    ``T.sigma``, the list's indices renamed in their entry order, the atom sets renamed, ``aromatic`` (by entry) kept."""
    n = len(m['types'])
    sigma = T.sigma(n, b)
    inverse = np.argsort(sigma)
    points = T.apply(m['points']).reshape(n, 3)
    rename = lambda atoms: sorted(int(sigma[k]) for k in atoms)      # noqa: E731
    return dict(types=[m['types'][k] for k in inverse], points=points[inverse],
                entries=[(int(sigma[i]), int(sigma[j]), o) + tuple(rest) for i, j, o, *rest in m['entries']],
                planar=rename(m['planar']), marked=rename(m['marked']), dropped=rename(m['dropped']), aromatic=list(m['aromatic']),
                sigma=sigma)


def pack(molecules, width, seed, nf=8, capacity=None):
    """The arrays of the bond-list entry points, under the names of both families of launch helpers: every molecule on
    ``width`` rows, scattered among rows that are not real and hold garbage (NaN included), its list in the first rows of
    ``capacity``.  ``planar`` is by atom number, ``marked`` and ``dropped`` become masks by row, ``aromatic`` flags by entry."""
    rng = np.random.default_rng(seed)
    B = len(molecules)
    capacity = max([len(m['entries']) for m in molecules] + [1]) + 2 if capacity is None else capacity
    x = rng.normal(0, 3, (B, width, 3)).astype(np.float32)
    x[rng.random((B, width)) < 0.3] = np.nan
    out = dict(x=x, one_hot=rng.random((B, width, nf)).astype(np.float32) * 0.5, mask=np.zeros((B, width), np.float32),
               drop=(rng.random((B, width)) < 0.3).astype(np.float32), mark=(rng.random((B, width)) < 0.3).astype(np.float32),
               planar=np.zeros((B, width), np.int32), bonds=np.full((B, capacity, 3), 7, np.int32), n_in=np.zeros(B, np.int32),
               status=np.zeros(B, np.int32), bond_aromatic=np.zeros((B, capacity), np.int32), rows=[], sigma=[])
    for b, m in enumerate(molecules):
        n = len(m['types'])
        rows = np.sort(rng.choice(width, n, replace=False))
        out['rows'].append(rows)
        out['sigma'].append(m.get('sigma', np.arange(n)))
        out['mask'][b, rows] = 1
        out['x'][b, rows] = np.asarray(m['points'], dtype=np.float64).reshape(n, 3)       # the one rounding to fp32
        out['one_hot'][b, rows] = 0
        out['one_hot'][b, rows, m['types']] = 1
        for key, atoms in (('drop', m['dropped']), ('mark', m['marked'])):
            out[key][b, rows] = 0
            out[key][b, rows[np.asarray(atoms, dtype=int)]] = 1
        out['planar'][b, np.asarray(m['planar'], dtype=int)] = 1
        for e, entry in enumerate(m['entries']):
            out['bonds'][b, e] = entry[:3]
        out['n_in'][b] = len(m['entries'])
        out['bond_aromatic'][b, np.asarray(m['aromatic'], dtype=int)] = 1
    out.update(node_mask=out['mask'], drop_mask=out['drop'], mark_mask=out['mark'], atom_planar=out['planar'],
               n_bonds_in=out['n_in'], status_in=out['status'])
    return out


def build_molecules(case, T, nf=8):
    molecules = [moved(m, T, b) for b, m in enumerate(case['molecules'])]
    return pack(molecules, case['width'], case['pack_seed'] + (T.seed if T.kind == 'renumber' else 0), nf=nf)


def by_atom(array_b, sigma):
    """Row ``b`` of an output indexed by atom number, put back into the base numbering."""
    return np.asarray(array_b)[np.asarray(sigma)]


def renamed_back(records, sigma, places=(0, 1)):
    """A multiset of records whose fields ``places`` are atom numbers of the renumbered molecule, in the base numbering."""
    inverse = np.argsort(sigma)
    out = []
    for r in records:
        r = list(r)
        for p in places:
            r[p] = int(inverse[r[p]])
        out.append(tuple(r))
    return sorted(out)


def same(a, b, what):
    assert np.array_equal(np.asarray(a), np.asarray(b)), (what, np.asarray(a).tolist(), np.asarray(b).tolist())


def close(a, b, limit, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    both = np.isinf(a) & (a == b)
    with np.errstate(invalid='ignore'):
        worst = float(np.abs(np.where(both, 0.0, a - b)).max(initial=0.0))
    assert worst <= limit, (what, worst, limit)
    return worst


# ---- the hand molecules on the axes: perp() and the plane fits on their axis-aligned inputs -------------------------------------
def axis_molecules():
    C, N_, O = pr.C, pr.N_, pr.O
    chain_z = [(0.0, 0.0, 1.5 * k) for k in range(5)]
    ring_xy = pr.polygon(6, 1.38)                    # not 1.39: the C=C bound of the distance table is 139 pm
    return [molecule_of([C] * 5, chain_z, pr.chain_bonds(5), marked=[1, 2, 3]),
            molecule_of([C] * 6, ring_xy, [((k + 1) % 6, k, 2 - k % 2) for k in range(6)], planar=range(6), marked=range(6),
                        aromatic=range(6)),
            molecule_of([C, N_], [(0.0, 0.0, 0.0), (1.16, 0.0, 0.0)], [(1, 0, 3)], marked=[1]),
            molecule_of([C, C, O], [(0.0, 1.5, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.43)], [(1, 0, 1), (2, 1, 1)], marked=[1, 2]),
            molecule_of([C, C, C], [(-1.25, 0.0, 0.0), (0.0, 0.0, 0.0), (1.25, 0.0, 0.0)], [(1, 0, 2), (2, 1, 2)], marked=[1]),
            molecule_of([N_], [(0.5, -1.0, 2.0)], marked=[0])]


# =================================================================================================================================
# ENTRY POINTS.  Each class states: the transforms applied, the outputs compared exactly, those compared within a bar, its
# cases and their fixed seeds.  ``build(case, T)`` makes the inputs, ``reference(inputs)`` runs the restatement, ``margins``
# lists the decision distances of the clearance, ``compare`` undoes ``T`` and compares two results of ONE implementation.
# =================================================================================================================================
class Entry:
    name = ''
    transforms = ALL
    runs = (None,)                 # variants of one launch (``steps`` of the relaxation)
    SEEDS = {}                     # the seeds found and fixed
    START = {}                     # where the search began, when not at the seed itself

    def cases(self):
        raise NotImplementedError

    def transforms_of(self, case_name):
        return self.transforms

    def case(self, name):
        if not hasattr(self, '_cases'):
            self._cases = self.cases()
        return self._cases[name]

    def case_names(self):
        if not hasattr(self, '_cases'):
            self._cases = self.cases()
        return list(self._cases)

    def build(self, case, T):
        return build_molecules(case, T)

    def runs_of(self, case_name):
        return self.runs

    def margins(self, inputs, run=None):
        return []


def first_clear_seed(entry, make, seed, tries=40):
    """The first of ``seed, seed + 100, ...`` whose case clears under every transform of the entry point."""
    for k in range(tries):
        case = make(seed + 100 * k)
        if all(min([m for _, m in entry.margins(entry.build(case, T))] + [math.inf]) >= MARGIN for T in [IDENTITY] + list(entry.transforms)):
            return seed + 100 * k, case
    raise AssertionError(f'{entry.name}: no seed of {seed}, {seed + 100}, ... clears')


def fixed_case(entry, name, make):
    """The case of the seed fixed in ``entry.SEEDS``, which must be the first of ``START`` (or itself), + 100, ... that clears."""
    found, case = first_clear_seed(entry, make, entry.START.get(name, entry.SEEDS[name]))
    assert found == entry.SEEDS[name], (entry.name, name, found, entry.SEEDS[name])
    return case


def real_molecule(inputs, b):
    """``(rows, types, fp64 points)`` of molecule ``b``'s real atoms in atom order."""
    rows = np.flatnonzero(inputs['mask'][b])
    return rows, np.argmax(inputs['one_hot'][b, rows], axis=1), inputs['x'][b, rows].astype(np.float64)


def kept_atoms(inputs, b, use_drop=True):
    rows = np.flatnonzero(inputs['mask'][b])
    return [k for k, r in enumerate(rows) if not (use_drop and inputs['drop'][b, r] != 0)]


# ---- dl_perceive_bonds ---------------------------------------------------------------------------------------------------------
class Bonds(Entry):
    """Transforms: all.  Exact: the bond list as a set of (lo, hi, order), n_bonds, valence, the components as a partition,
    n_components, status.  No continuous output.  Restatement: ``pose_checks_ref.perceive`` (the distance table in fp64)."""
    name = 'dl_perceive_bonds'
    SEEDS = {'random': 301, 'small': 302}

    def make_random(self, seed, count=8, max_atoms=30):
        rng = np.random.default_rng(seed)
        molecules = []
        while len(molecules) < count:
            m = pr.random_molecule(rng, max_atoms)
            m = molecule_of(m['types'], m['points'])
            if min([d for _, d in self.molecule_margins(m['types'], m['points'])] + [math.inf]) >= 2 * MARGIN:
                molecules.append(m)
        return dict(molecules=molecules, width=max_atoms + 3, pack_seed=seed)

    def cases(self):
        axes = [molecule_of(m['types'], m['points']) for m in axis_molecules()]
        return {'random': self.make_random(self.SEEDS['random']), 'small': self.make_random(self.SEEDS['small'], 16, 9),
                'axes': dict(molecules=axes, width=8, pack_seed=3)}

    @staticmethod
    def molecule_margins(types, points):
        from difflinker_amd.const import BOND_LENGTHS, MARGINS_EDM
        p = f32(points)
        out = []
        for i in range(len(types)):
            for j in range(i):
                d = 100.0 * math.sqrt(float(((p[i] - p[j]) ** 2).sum()))
                for k in range(3):
                    if BOND_LENGTHS[k][types[i]][types[j]]:
                        out.append((('bond', i, j, k), abs(d - (BOND_LENGTHS[k][types[i]][types[j]] + MARGINS_EDM[k])) / 100.0))
        return out

    def margins(self, inputs, run=None):
        out = []
        for b in range(len(inputs['mask'])):
            _, types, points = real_molecule(inputs, b)
            out += self.molecule_margins(types.tolist(), points)
        return out

    def reference(self, inputs, run=None):
        B, N = inputs['mask'].shape
        out = dict(bonds=[], n_bonds=np.zeros(B, np.int32), valence=np.zeros((B, N), np.int32), component=np.full((B, N), -1, np.int32),
                   n_components=np.zeros(B, np.int32), status=np.zeros(B, np.int32))
        for b in range(B):
            _, types, points = real_molecule(inputs, b)
            found = pr.perceive(types.tolist(), points)
            out['bonds'].append(found)
            out['n_bonds'][b] = len(found)
            label = list(range(len(types)))
            for i, j, order in found:
                out['valence'][b, i] += order
                out['valence'][b, j] += order
                lo, hi = sorted((label[i], label[j]))
                label = [lo if v == hi else v for v in label]
            out['component'][b, :len(types)] = label
            out['n_components'][b] = len(set(label))
        return out

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        for name in ('n_bonds', 'n_components', 'status'):
            same(out0[name], out1[name], name)
        for b, sigma in enumerate(in1['sigma']):
            n = len(sigma)
            pairs = lambda rows: sorted((min(i, j), max(i, j), o) for i, j, o in rows)       # noqa: E731
            assert pairs(out0['bonds'][b]) == pairs(renamed_back(out1['bonds'][b], sigma)), ('bonds', b)
            same(out0['valence'][b, :n], by_atom(out1['valence'][b], sigma), ('valence', b))
            same(out0['valence'][b, n:], out1['valence'][b, n:], ('valence beyond the atoms', b))
            groups = lambda labels: sorted(sorted(np.flatnonzero(labels == v).tolist()) for v in set(labels.tolist()))   # noqa: E731
            assert groups(out0['component'][b, :n]) == groups(by_atom(out1['component'][b], sigma)), ('component', b)


# ---- dl_pose_checks -------------------------------------------------------------------------------------------------------------
class PoseChecks(Entry):
    """Transforms: all (lengths, angles and clashes are torsion-free: no handedness).  Exact: counts, atom_flags by atom
    number, status.  No continuous output."""
    name = 'dl_pose_checks'
    SEEDS = {'random': 311, 'hand': 0}

    def make_random(self, seed, count=8, max_atoms=30):
        rng = np.random.default_rng(seed)
        molecules = []
        while len(molecules) < count:
            m = pr.random_molecule(rng, max_atoms)
            m = molecule_of(**m)
            one = dict(molecules=[m], width=len(m['types']) + 2, pack_seed=1)
            if min([d for _, d in self.margins(build_molecules(one, IDENTITY))] + [math.inf]) >= 2 * MARGIN:
                molecules.append(m)
        return dict(molecules=molecules, width=max_atoms + 3, pack_seed=seed)

    def cases(self):
        hand = [molecule_of(**pr.hand_molecule(name)) for name in sorted(pr.HAND)][:MAX_B]
        for m in hand:
            m['marked'] = list(range(1, len(m['types'])))
        return {'random': self.make_random(self.SEEDS['random']), 'hand': dict(molecules=hand, width=9, pack_seed=4),
                'axes': dict(molecules=axis_molecules(), width=8, pack_seed=3)}

    def margins(self, inputs, run=None):
        bounds2, cosines, clashes2 = pr.default_tables()
        out = []
        for b in range(len(inputs['mask'])):
            detail = {}
            pr.molecule(inputs['x'][b], np.argmax(inputs['one_hot'][b], axis=1), inputs['mask'][b], inputs['bonds'][b],
                        int(inputs['n_in'][b]), bounds2, cosines, clashes2, 0, inputs['drop'][b], inputs['mark'][b], inputs['planar'][b],
                        detail=detail)
            rows = np.flatnonzero(inputs['mask'][b])
            kind = np.argmax(inputs['one_hot'][b, rows], axis=1)
            for a, j, order, d2, verdict in detail['bonds']:
                if d2 is not None:
                    for bound in bounds2[kind[a]][kind[j]][order - 1]:
                        out.append((('length', b, a, j), abs(math.sqrt(d2) - math.sqrt(bound))))
            for j, a, k, cls, c, _ in detail['angles']:
                for bound in cosines[cls]:
                    if -1.0 <= bound <= 1.0:
                        out.append((('cosine', b, j, a, k), abs(c - bound) * MARGIN / COS_MARGIN))
            for a, c, d2, _ in detail['pairs']:
                if clashes2[kind[a]][kind[c]] > 0:
                    out.append((('clash', b, a, c), abs(math.sqrt(d2) - math.sqrt(clashes2[kind[a]][kind[c]]))))
        return out

    def reference(self, inputs, run=None):
        return pr.pose_checks(inputs['x'], inputs['one_hot'], inputs['mask'], inputs['bonds'], inputs['n_in'], *pr.default_tables(),
                              inputs['status'], inputs['drop'], inputs['mark'], inputs['planar'])

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        same(out0['counts'], out1['counts'], 'counts')
        same(out0['status'], out1['status'], 'status')
        for b, sigma in enumerate(in1['sigma']):
            n = len(sigma)
            same(out0['atom_flags'][b, :n], by_atom(out1['atom_flags'][b], sigma), ('atom_flags', b))
            same(out0['atom_flags'][b, n:], out1['atom_flags'][b, n:], ('atom_flags beyond the atoms', b))


# ---- dl_relax_molecules ---------------------------------------------------------------------------------------------------------
class Relax(Entry):
    """Transforms: all (no torsion term: no handedness), at ``steps`` 0, 1 and 40.  Exact: steps_done, status, and the rows of
    x_out that do not move (bit for bit the input).  Within ``RELAX_BAR_FACTOR`` x the restatement's measured deviation: x_out
    of the moved rows after the inverse motion (A), energy, f_max and moved2 (relative to max(1, |value|))."""
    name = 'dl_relax_molecules'
    runs = (0, 1, 40)
    SEEDS = {'random': 321, 'axes': 0}

    def make_random(self, seed, count=6, max_atoms=16):
        rng = np.random.default_rng(seed)
        molecules = []
        while len(molecules) < count:
            m = molecule_of(**pr.random_molecule(rng, max_atoms, min_atoms=3))
            one = dict(molecules=[m], width=len(m['types']) + 2, pack_seed=1)
            if min([d for _, d in self.margins(build_molecules(one, IDENTITY))] + [math.inf]) >= 2 * MARGIN:
                molecules.append(m)
        return dict(molecules=molecules, width=max_atoms + 3, pack_seed=seed)

    @staticmethod
    def axis_molecules(seed):
        """Strained molecules on an axis or in a coordinate plane, large enough not to settle in 40 steps, and STRETCHED: a
        compressed chain on an axis sits on a saddle, where the rounding of a rotated input decides which way it buckles and
        two frames part by 0.03 A in 40 steps - a property of the minimisation, not of an implementation.  Twelve carbons along
        z at uneven spacings, a chain of fourteen atoms folded at random in the xy plane, eight cumulated carbons along x, and
        a six-ring in the xy plane with every atom at another distance from the centre."""
        rng = np.random.default_rng(seed)
        C, N_, O = pr.C, pr.N_, pr.O
        z = np.cumsum(rng.uniform(1.6, 2.1, 12))
        out = [molecule_of([C] * 12, np.stack([0 * z, 0 * z, z], 1), pr.chain_bonds(12), marked=range(1, 11))]
        walk = [(0.0, 0.0)]
        for _ in range(13):
            angle, step = rng.uniform(0, 2 * math.pi), rng.uniform(1.6, 2.1)
            walk.append((walk[-1][0] + step * math.cos(angle), walk[-1][1] + step * math.sin(angle)))
        out.append(molecule_of([C, C, N_, C, O, C, C] * 2, [(x, y, 0.0) for x, y in walk], pr.chain_bonds(14), marked=range(2, 13),
                               planar=[3, 4]))
        x = np.cumsum(rng.uniform(1.4, 1.7, 8))
        out.append(molecule_of([C] * 8, np.stack([x, 0 * x, 0 * x], 1), [(k + 1, k, 2) for k in range(7)], marked=range(1, 7)))
        ring = np.array(pr.polygon(6, 1.38)) * rng.uniform(1.05, 1.25, (6, 1))
        out.append(molecule_of([C] * 6, ring, [((k + 1) % 6, k, 2 - k % 2) for k in range(6)], planar=range(6), marked=range(6),
                               aromatic=range(6)))
        return out

    def cases(self):
        """Every case runs 0, 1 and 40 steps and none of its molecules settles within 40."""
        hand = [molecule_of(**m) for m in (rr.perturbed_chain(), rr.perturbed_chain(9, 0.25, 6), rr.folded_linker(), rr.walled())]
        return {'random': self.make_random(self.SEEDS['random']), 'hand': dict(molecules=hand, width=14, pack_seed=5),
                'axes': dict(molecules=self.axis_molecules(self.SEEDS['axes']), width=16, pack_seed=3)}

    def margins(self, inputs, run=None):
        """The one threshold of the iteration: ``f < f_tol`` ends a run, ``f`` the largest |F| of a movable atom.  A
        displacement of ``MARGIN`` changes the force of one bond by ``2 k_bond MARGIN``, so the ``f`` of every step of the run,
        divided by ``2 k_bond``, must stay ``MARGIN`` away from ``f_tol``: ``f_tol`` = 1e-3 is the force of a bond 5e-6 A off
        its length, below the rounding of a coordinate at 300 A, so no molecule of these cases converges within its steps and
        the exit itself is shown in two frames by ``test_relax_f_is_a_length`` on coordinates where it is exact.  (A molecule
        without a movable atom has no force; its run ends at once in every frame.)"""
        seen, original = [], rr.Molecule.forces

        def recorder(mol, x):
            F = original(mol, x)
            if len(mol.M):
                seen.append(float(np.sqrt(rr.dot(F[mol.M], F[mol.M])).max()))
            return F

        rr.Molecule.forces = recorder
        try:
            self.reference(inputs, max(self.runs) if run is None else run)
        finally:
            rr.Molecule.forces = original
        stiff = 2.0 * rr.DEFAULTS['k_bond']
        return [(('f_tol', k), abs(f - rr.DEFAULTS['f_tol']) / stiff) for k, f in enumerate(seen)]

    def reference(self, inputs, run=0):
        return rr.relax(inputs['x'], inputs['one_hot'], inputs['mask'], inputs['bonds'], inputs['n_in'], rr.default_tables(),
                        inputs['bond_aromatic'], inputs['status'], inputs['drop'], inputs['mark'], inputs['planar'], True, run)

    def deviations(self, T, in0, out0, in1, out1):
        """The largest deviation of every continuous output: ``x`` of the moved rows after the inverse motion, in A; ``energy``,
        ``f_max`` and ``moved2`` relative to max(1, |value|)."""
        dx = 0.0
        for b, sigma in enumerate(in1['sigma']):
            rows0, rows1 = in0['rows'][b], in1['rows'][b]
            if len(sigma):
                back = T.undo(out1['x_out'][b, rows1[sigma]])
                dx = max(dx, float(np.abs(back - out0['x_out'][b, rows0]).max()))
        relative = lambda name: float((np.abs(out0[name] - out1[name]) / np.maximum(1.0, np.abs(out0[name]))).max(initial=0.0))   # noqa: E731
        return dict(x=dx, energy=relative('energy'), f_max=relative('f_max'), moved2=relative('moved2'))

    def compare(self, case, T, in0, out0, in1, out1, run=0, factor=RELAX_BAR_FACTOR):
        same(out0['steps_done'], out1['steps_done'], 'steps_done')
        same(out0['status'], out1['status'], 'status')
        for b, sigma in enumerate(in1['sigma']):
            rows1 = in1['rows'][b]
            fixed = [r for r in rows1 if in1['mark'][b, r] == 0 or in1['drop'][b, r] != 0]
            assert out1['x_out'][b, fixed].tobytes() == in1['x'][b, fixed].tobytes(), ('an unmarked row comes back bit for bit', b)
        found = self.deviations(T, in0, out0, in1, out1)
        for name, value in found.items():
            assert value <= factor * RELAX_DEVIATION[run][name], (name, value, RELAX_DEVIATION[run][name], factor)
        return found


# ---- dl_add_hydrogens -----------------------------------------------------------------------------------------------------------
class Hydrogens(Entry):
    """Transforms: all.  Exact: n_h, h_count by atom number, the parents as a multiset, status.  Within the bar: h_x after the
    inverse motion, matched per parent.

    The rule fills the sites of an atom in a fixed order, and two of its choices are not fixed by the geometry alone; both are
    the header's own words, and ``site_kind`` names them per parent from the bond graph:
      'handed'    T4 with two neighbours and one hydrogen, T4 with one neighbour and two hydrogens, T4 with three neighbours
                  in a plane: ``n = u1 x u2``, ``e2 = u1 x e1`` and ``w = (u2 - u1) x (u3 - u1)`` carry the hand of the frame
                  and the order of the neighbours.  Under a mirror, and under
                  a renumbering that swaps the neighbours, the hydrogen sits on the OTHER free site: the mirror image of the
                  base hydrogen in the plane of the atom and its reference directions.  That image is what is compared: a
                  full comparison still.
      'numbered'  one neighbour k that has two or more other neighbours: "r the smallest-numbered neighbour of k other than
                  a" - under a renumbering only the frame-free content is compared for such a parent.
      'arbitrary' ``perp(u)`` and the fixed directions of a lone atom (``FRAME_DEPENDENT_BY_RULE``): frame-free content only."""
    name = 'dl_add_hydrogens'
    SEEDS = {'random': 331}

    def make_random(self, seed, count=8, max_atoms=30):
        rng = np.random.default_rng(seed)
        molecules = []
        while len(molecules) < count:
            (m,), _ = hr.random_molecules(rng, 1, max_atoms, with_drop=lambda b: True)
            m = molecule_of(**m)
            if len(m['types']) < 2:
                continue
            one = dict(molecules=[m], width=len(m['types']) + 2, pack_seed=1)
            inputs = build_molecules(one, IDENTITY)
            kinds = self.site_kinds(inputs, 0)
            if 'arbitrary' in kinds.values() or min([d for _, d in self.margins(inputs)] + [math.inf]) < 2 * MARGIN:
                continue
            molecules.append(m)
        return dict(molecules=molecules, width=max_atoms + 3, pack_seed=seed)

    def cases(self):
        names = ('propane', 'dimethylamine', 'isobutane', 'propene', 'benzene', 'pyrrole', 'sulfone', 'trigonal_planar')
        hand = [molecule_of(**hr.hand_molecule(n)) for n in names]
        return {'random': self.make_random(self.SEEDS['random']), 'hand': dict(molecules=hand, width=8, pack_seed=6),
                'axes': dict(molecules=axis_molecules() + [molecule_of(**hr.hand_molecule(n)) for n in ('ethane', 'methanol', 'methylamine', 'antiparallel', 't_shaped', 'lone_C')],
                             width=8, pack_seed=3)}

    @staticmethod
    def graph(inputs, b):
        """``(kept, adj, orders)`` of molecule ``b`` by atom number, as the rule builds them."""
        kept = set(kept_atoms(inputs, b))
        adj, orders = {k: [] for k in kept}, {}
        for i, j, o in inputs['bonds'][b, :inputs['n_in'][b]].tolist():
            if i in kept and j in kept and (min(i, j), max(i, j)) not in orders:
                orders[(min(i, j), max(i, j))] = o
                adj[i].append(j)
                adj[j].append(i)
        return kept, {k: sorted(v) for k, v in adj.items()}, orders

    def site_kinds(self, inputs, b, decisions=None):
        """parent atom -> 'full', 'handed', 'numbered', 'handed+numbered' or 'arbitrary', from the graph and the ``EPS``
        branches taken."""
        valence, _ = hr.tables()
        kept, adj, orders = self.graph(inputs, b)
        rows, types, points = real_molecule(inputs, b)
        pos = {k: tuple(points[k]) for k in kept}
        out = {}
        for a in sorted(kept):
            o = [orders[(min(a, t), max(a, t))] for t in adj[a]]
            d, h0 = len(o), max(0, int(valence[types[a]]) - sum(o))
            n2, n3 = o.count(2), o.count(3)
            cls = hr.T2 if n3 or n2 >= 2 else hr.T3 if n2 == 1 or (inputs['planar'][b, a] != 0 and d == 2 and h0 == 1) else hr.T4
            h = min(h0, max(0, cls - d))
            if h == 0:
                continue
            taken = []
            hr.directions(a, pos, adj, cls, d, taken)
            perp = d == 0 or any((name == 'p.p / w.w' and not value > limit) or (name in ('s.s',) and d == 2 and value <= limit) or
                                 (name == 'c.c' and not value > limit) or (name == 'w.w' and not value > limit)
                                 for name, value, limit in taken)
            others = [t for t in adj[adj[a][0]] if t != a] if d == 1 else []
            arbitrary = perp or (d == 1 and not others and cls != hr.T2)
            handed = cls == hr.T4 and ((d == 2 and h == 1) or (d == 1 and h == 2) or (d == 3 and any(name == 'w.w' for name, _, _ in taken)))
            numbered = d == 1 and cls != hr.T2 and len(others) >= 2
            out[a] = 'arbitrary' if arbitrary else '+'.join(['handed'] * handed + ['numbered'] * numbered) or 'full'
        return out

    def margins(self, inputs, run=None):
        """The ``EPS`` branches: ``hydrogens_ref.near_threshold`` keeps every quantity a factor 10 from ``EPS``; here the same
        quantities as sines: sqrt(value) is the sine of an angle (or twice the cosine of a half angle), so a factor 10 in the
        value is a factor 3 in an angle of 1e-3 rad - far beyond a displacement of 1e-3 A on arms of 1 A."""
        valence, length = hr.tables()
        out = []
        for b in range(len(inputs['mask'])):
            decisions = []
            hr.molecule(inputs['x'][b], np.argmax(inputs['one_hot'][b], axis=1), inputs['mask'][b], inputs['bonds'][b],
                        int(inputs['n_in'][b]), valence, length, 0, inputs['drop'][b], inputs['planar'][b], decisions=decisions)
            for name, value, limit in decisions:
                near = not (value < limit / 10.0 or value > limit * 10.0)
                exact = value == 0.0                                    # an exact degenerate input stays one under exact transforms
                out.append((('EPS', b, name), 0.0 if near and not exact else math.inf))
        return out

    def reference(self, inputs, run=None):
        valence, length = hr.tables()
        return hr.add_hydrogens(inputs['x'], inputs['one_hot'], inputs['mask'], inputs['bonds'], inputs['n_in'], valence, length,
                                4 * inputs['mask'].shape[1], inputs['status'], inputs['drop'], inputs['planar'])

    @staticmethod
    def listed(out, b):
        n = int(out['n_h'][b])
        return out['h_parent'][b, :n], out['h_x'][b, :n]

    @staticmethod
    def frame_free(xa, hs, neighbours):
        """X-H lengths, H-X-H and H-X-neighbour angles (as cosines), each sorted."""
        v = [h - xa for h in hs]
        u = [p - xa for p in neighbours]
        cos = lambda p, q: float(p @ q) / math.sqrt(float(p @ p) * float(q @ q))        # noqa: E731
        return (sorted(math.sqrt(float(p @ p)) for p in v), sorted(cos(p, q) for k, p in enumerate(v) for q in v[:k]),
                sorted(cos(p, q) for p in v for q in u))

    def compare(self, case, T, in0, out0, in1, out1, run=None, case_name=None):
        same(out0['n_h'], out1['n_h'], 'n_h')
        same(out0['status'], out1['status'], 'status')
        by_rule = case_name in FRAME_DEPENDENT_BY_RULE.get(self.name, {}).get('cases', ())
        worst = 0.0
        for b, sigma in enumerate(in1['sigma']):
            n = len(sigma)
            same(out0['h_count'][b, :n], by_atom(out1['h_count'][b], sigma), ('h_count', b))
            same(out0['h_count'][b, n:], out1['h_count'][b, n:], ('h_count beyond the atoms', b))
            p0, x0 = self.listed(out0, b)
            p1, x1 = self.listed(out1, b)
            inverse = np.argsort(sigma)
            assert sorted(p0.tolist()) == sorted(inverse[p1].tolist()), ('parents', b)
            assert np.all(np.diff(p1) >= 0), ('the list is by parent', b)
            kinds = self.site_kinds(in0, b)
            assert by_rule or 'arbitrary' not in kinds.values(), ('a case outside FRAME_DEPENDENT_BY_RULE uses perp()', b, kinds)
            _, adj, _ = self.graph(in0, b)
            _, _, pts0 = real_molecule(in0, b)
            _, _, pts1 = real_molecule(in1, b)
            limit = bar(T, np.float64, x0 if len(x0) else [1.0], in0['x'][b, in0['rows'][b]], in1['x'][b, in1['rows'][b]],
                        entry=self.name, output='h_x')
            for a in sorted(set(p0.tolist())):
                h0 = x0[p0 == a]
                h1_raw = x1[p1 == sigma[a]]
                free0 = self.frame_free(pts0[a], list(h0), [pts0[t] for t in adj[a]])
                free1 = self.frame_free(pts1[sigma[a]], list(h1_raw), [pts1[sigma[t]] for t in adj[a]])
                for f0, f1 in zip(free0, free1):
                    close(f0, f1, max(limit, 1e-12), ('frame-free content', b, a))
                kind = kinds[a]
                if kind == 'arbitrary' or ('numbered' in kind and T.kind == 'renumber'):
                    continue
                h1 = T.undo(h1_raw)
                if 'handed' in kind:
                    swapped = not T.proper
                    if T.kind == 'renumber' and len(adj[a]) >= 2:      # the parity of the neighbours' new order
                        new = [sigma[t] for t in adj[a]]
                        swapped = sum(p > q for k, q in enumerate(new) for p in new[:k]) % 2 == 1
                    if swapped:
                        h1 = self.other_site(pts0, a, adj, h1, h0)
                order = np.lexsort(np.round(h0, 6).T)
                order1 = np.lexsort(np.round(h1, 6).T)
                if T.kind == 'renumber' or 'handed' in kind or not T.proper:
                    worst = max(worst, close(h0[order], h1[order1], limit, ('h_x as a set', b, a, kind)))
                else:
                    worst = max(worst, close(h0, h1, limit, ('h_x in list order', b, a, kind)))
        return worst

    @staticmethod
    def other_site(pts, a, adj, h1, h0):
        """The hydrogens ``h1`` of a handed parent mirrored in the plane through the atom that holds its reference directions:
        the two neighbours (two neighbours) or the neighbour and the first, anti, hydrogen (one neighbour)."""
        xa = pts[a]
        if len(adj[a]) == 3:                          # w = (u2 - u1) x (u3 - u1) changes sign: the other side of the neighbours' plane
            return 2.0 * xa - h1
        if len(adj[a]) == 2:
            p, q = pts[adj[a][0]] - xa, pts[adj[a][1]] - xa
        else:
            p, q = pts[adj[a][0]] - xa, h0[0] - xa
        normal = np.cross(p, q)
        normal = normal / np.linalg.norm(normal)
        return h1 - 2.0 * ((h1 - xa) @ normal)[:, None] * normal[None, :]


# ---- dl_aromatic_rings ----------------------------------------------------------------------------------------------------------
class Aromatic(Entry):
    """Transforms: all (planarity has no handedness).  Exact: n_planar_rings, n_aromatic_rings, n_aromatic_marked, status,
    atom_aromatic by atom number, bond_aromatic by entry; and, except under a renumbering, order_out by entry and valence_out by
    atom number - the Kekule assignment is by definition "the smallest sorted list of (min, max) pairs" among equals, which is
    the numbering's and moves with it (aromaticity of a ring whose every carbon is covered does not).  No continuous output."""
    name = 'dl_aromatic_rings'
    SEEDS = {'fused': 341}

    def make_random(self, seed, count=8):
        rng = np.random.default_rng(seed)
        molecules = []
        while len(molecules) < count:
            types, points, entries = ar.random_fused(rng, MAX_ATOMS)
            m = molecule_of(types, points, entries, marked=[k for k in range(len(types)) if rng.random() < 0.7])
            one = dict(molecules=[m], width=len(types) + 2, pack_seed=1)
            if min([d for _, d in self.margins(build_molecules(one, IDENTITY))] + [math.inf]) >= 2 * MARGIN:
                molecules.append(m)
        return dict(molecules=molecules, width=MAX_ATOMS + 3, pack_seed=seed)

    def cases(self):
        hand = [molecule_of(*ar.hand_molecule(name)) for name in sorted(ar.HAND)][:MAX_B]
        return {'fused': self.make_random(self.SEEDS['fused']), 'hand': dict(molecules=hand, width=14, pack_seed=7),
                'axes': dict(molecules=axis_molecules(), width=8, pack_seed=3)}

    def margins(self, inputs, run=None):
        """Every candidate ring's atoms and substituents: their distance |d| / |m| from the ring's plane against the two
        tolerances (the rule compares d^2 with tol^2 * m.m), and the ring's area vector against 0."""
        out, original = [], ar.is_planar

        def recorder(cycle, adj, pos, tol2_ring=ar.TOL2_RING, tol2_sub=ar.TOL2_SUB):
            c, q, m, mm = ar.ring_plane([pos[k] for k in cycle])
            out.append((('area', cycle), math.sqrt(mm)))
            if mm > 0:
                for v in q:
                    out.append((('ring atom', cycle), abs(abs(ar.dot(v, m)) / math.sqrt(mm) - math.sqrt(tol2_ring))))
                for k in cycle:
                    for s in adj[k]:
                        if s not in cycle:
                            d = ar.dot(tuple(pos[s][t] - c[t] for t in range(3)), m)
                            out.append((('substituent', cycle, s), abs(abs(d) / math.sqrt(mm) - math.sqrt(tol2_sub))))
            return original(cycle, adj, pos, tol2_ring, tol2_sub)

        ar.is_planar = recorder
        try:
            self.reference(inputs)
        finally:
            ar.is_planar = original
        return out

    def reference(self, inputs, run=None):
        return ar.aromatic_rings(inputs['x'], inputs['one_hot'], inputs['mask'], inputs['bonds'], inputs['n_in'],
                                 ar.ring_class_table(hr.ATOM2IDX), inputs['status'], inputs['drop'], inputs['mark'])

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        names = ['n_planar_rings', 'n_aromatic_rings', 'n_aromatic_marked', 'status', 'bond_aromatic']
        for name in names + ([] if T.kind == 'renumber' else ['order_out']):
            same(out0[name], out1[name], name)
        for b, sigma in enumerate(in1['sigma']):
            n = len(sigma)
            for name in ['atom_aromatic'] + ([] if T.kind == 'renumber' else ['valence_out']):
                same(out0[name][b, :n], by_atom(out1[name][b], sigma), (name, b))
                same(out0[name][b, n:], out1[name][b, n:], (name, 'beyond the atoms', b))
            if T.kind == 'renumber':                                    # every Kekule assignment has the same number of double bonds
                ring = out0['order_out'][b] != in0['bonds'][b, :, 2]
                assert sorted(out0['valence_out'][b, :n].tolist()) == sorted(out1['valence_out'][b, :n].tolist()) or ring.any()
                assert int(out0['valence_out'][b].sum()) == int(out1['valence_out'][b].sum()), ('the sum of the orders', b)


# ---- rows with masks: dl_clash_scores, dl_interaction_types, dl_interaction_scores ------------------------------------------------
NF9 = 9


def protein_257(seed, centre, near=12):
    """A shared list of 257 atoms (one past the tile of 256): ``near`` of them in the molecules' box, the others 15 to 40 A
    away, so that few pairs lie next to a threshold."""
    rng = np.random.default_rng(seed)
    direction = rng.normal(size=(257, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    x = centre + direction * rng.uniform(15.0, 40.0, (257, 1))
    x[rng.choice(257, near, replace=False)] = centre + rng.uniform(-4.0, 4.0, (near, 3))
    weights = np.array([5, 3, 3] + [0.4] * (NF9 - 3))
    return f32(x), rng.choice(NF9, size=257, p=weights / weights.sum()).astype(np.int64)


def row_batch(seed, B=4, N=24, n_query=5, n_ligand=9, n_pocket=10, box=6.0, centre=(20.0, 20.0, 20.0)):
    """Rows in random order as ``test_gpu_interaction.molecule`` lays them out: ligand rows of which some are queries, pocket
    rows, padding with finite garbage.  Returns ``dict(x, types, qm, lig, tm)`` with fp32-valued fp64 coordinates."""
    rng = np.random.default_rng(seed)
    weights = np.array([5, 3, 3] + [0.4] * (NF9 - 3))
    out = dict(x=f32(np.asarray(centre) + rng.uniform(-box / 2, box / 2, (B, N, 3))),
               types=rng.choice(NF9, size=(B, N), p=weights / weights.sum()), qm=np.zeros((B, N), np.float32),
               lig=np.zeros((B, N), np.float32), tm=np.zeros((B, N), np.float32))
    for b in range(B):
        rows = rng.permutation(N)
        nq, nl = n_query + b % 3, n_ligand + b % 4
        out['qm'][b, rows[:nq]] = 1
        out['lig'][b, rows[:nl]] = 1
        out['tm'][b, rows[nl:nl + n_pocket]] = 1
    return out


def build_rows(case, T):
    """The row arrays under ``T``: a renumbering permutes the rows of every molecule (masks and types go along) and,
    independently, the shared protein list."""
    B, N = case['qm'].shape
    out = dict(sigma=[T.sigma(N, b) for b in range(B)])
    for name in ('x', 'types', 'qm', 'lig', 'tm'):
        moved_rows = np.empty_like(case[name] if name != 'x' else np.zeros((B, N, 3), np.float32))
        source = T.apply(case['x']).astype(np.float32) if name == 'x' else case[name]
        for b, sigma in enumerate(out['sigma']):
            moved_rows[b, sigma] = source[b]
        out[name] = moved_rows
    out['one_hot'] = np.eye(NF9, dtype=np.float32)[out['types']]
    out['group'] = (out['lig'] != 0).astype(np.int32) + 2 * ((out['tm'] != 0) & (out['lig'] == 0)).astype(np.int32)
    if 'protein_x' in case:
        tau = T.sigma(len(case['protein_x']), 0, salt=1)
        out['tau'] = tau
        out['protein_x'] = np.empty((len(tau), 3), np.float32)
        out['protein_x'][tau] = T.apply(case['protein_x']).astype(np.float32)
        out['protein_type'] = np.empty(len(tau), np.int64)
        out['protein_type'][tau] = case['protein_type']
    return out


def pair_distances(inputs, b, with_protein=True):
    """``(q rows, distances [nq, nt], target types)`` of molecule ``b`` in fp64: own targets first, then the shared list."""
    qm = inputs['qm'][b] != 0
    tm = (inputs['tm'][b] != 0) & ~qm
    q = inputs['x'][b, qm].astype(np.float64)
    t = inputs['x'][b, tm].astype(np.float64)
    types = inputs['types'][b, tm]
    if with_protein and 'protein_x' in inputs:
        t = np.concatenate([t, inputs['protein_x'].astype(np.float64)])
        types = np.concatenate([types, inputs['protein_type']])
    return np.flatnonzero(qm), np.sqrt(((q[:, None] - t[None]) ** 2).sum(-1)), types


class Clash(Entry):
    """Transforms: all (distances only).  Exact: n_query, n_target, n_clashes, n_clash_atoms, n_contacts, status, atom_clashes
    by row.  Within the bar, as distances (the square roots of the fp32 outputs): min_dist2, atom_min_dist2 by row."""
    name = 'dl_clash_scores'
    SEEDS = {'own_targets': 351, 'shared_257': 352, 'both': 353}

    def make(self, seed, own=True, shared=False):
        case = row_batch(seed, n_pocket=10 if own else 0)
        if shared:
            case['protein_x'], case['protein_type'] = protein_257(seed + 1, np.array([20.0, 20.0, 20.0]))
        return case

    def cases(self):
        kinds = {'own_targets': (True, False), 'shared_257': (False, True), 'both': (True, True)}
        return {name: fixed_case(self, name, lambda s, k=k: self.make(s, *k)) for name, k in kinds.items()}

    def build(self, case, T):
        return build_rows(case, T)

    @staticmethod
    def thresholds():
        from difflinker_amd.const import VDW_RADII
        return np.array([[0.75 * (VDW_RADII[s] + VDW_RADII[t]) for t in range(NF9)] for s in range(NF9)])

    def margins(self, inputs, run=None):
        out, threshold = [], self.thresholds()
        for b in range(len(inputs['qm'])):
            rows, d, types = pair_distances(inputs, b)
            if d.size:
                limit = threshold[inputs['types'][b, rows][:, None], types[None, :]]
                out.append((('clash', b), float(np.abs(d - limit).min())))
                out.append((('contact', b), float(np.abs(d - 4.0).min())))
        return out

    def reference(self, inputs, run=None):
        from difflinker_amd import const
        return clash_ref.clash_scores(inputs['x'], inputs['one_hot'], inputs['qm'], const.clash_threshold_table(True).numpy(), inputs['tm'],
                                      inputs.get('protein_x'), inputs.get('protein_type'))

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        for name in ('n_query', 'n_target', 'n_clashes', 'n_clash_atoms', 'n_contacts', 'status'):
            same(out0[name], out1[name], name)
        worst = 0.0
        for b, sigma in enumerate(in1['sigma']):
            same(out0['atom_clashes'][b], out1['atom_clashes'][b][sigma], ('atom_clashes', b))
            near0 = np.sqrt(np.append(out0['atom_min_dist2'][b].astype(np.float64), out0['min_dist2'][b]))
            near1 = np.sqrt(np.append(out1['atom_min_dist2'][b][sigma].astype(np.float64), out1['min_dist2'][b]))
            limit = bar(T, np.float32, near0[np.isfinite(near0)], in0['x'][b], in1['x'][b], in0.get('protein_x', np.zeros(1)),
                        in1.get('protein_x', np.zeros(1)))
            worst = max(worst, close(near0, near1, limit, ('nearest distances', b)))
        return worst


class InteractionTypes(Entry):
    """Transforms: all.  Exact: xs_type by row, status.  No continuous output."""
    name = 'dl_interaction_types'
    SEEDS = {'mixed': 361, 'dense': 362}

    def cases(self):
        return {'mixed': fixed_case(self, 'mixed', row_batch),
                'dense': fixed_case(self, 'dense', lambda s: row_batch(s, B=6, N=16, box=4.5))}

    def build(self, case, T):
        return build_rows(case, T)

    @staticmethod
    def table():
        from difflinker_amd import const
        return const.bond_threshold_table(True)[..., 0].numpy()

    def margins(self, inputs, run=None):
        out, table = [], self.table().astype(np.float64)
        for b in range(len(inputs['qm'])):
            rows = np.flatnonzero(inputs['group'][b])
            p, e, g = inputs['x'][b, rows].astype(np.float64), inputs['types'][b, rows], inputs['group'][b, rows]
            d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
            pairs = (g[:, None] == g[None, :]) & ~np.eye(len(rows), dtype=bool)
            if pairs.any():
                out.append((('neighbour', b), float(np.abs(d - table[e[:, None], e[None, :]] / 100.0)[pairs].min())))
                out.append((('hydroxyl', b), float(np.abs(d - math.sqrt(1.6875))[pairs].min())))
        return out

    def reference(self, inputs, run=None):
        xs, status = ir.interaction_types(inputs['x'], inputs['one_hot'], inputs['group'], self.table())
        return dict(xs_type=xs, status=status)

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        same(out0['status'], out1['status'], 'status')
        for b, sigma in enumerate(in1['sigma']):
            same(out0['xs_type'][b], out1['xs_type'][b][sigma], ('xs_type', b))


class InteractionScores(Entry):
    """Transforms: all.  ``xs_type`` is typed in the frame of the inputs (its decisions are part of the clearance); the shared
    list of case 'shared_257' can only be handed over through ``analyze_interactions``, which types with the kernel.  Exact:
    n_query, n_target, n_pairs, n_hbonds, n_hydrophobic, status.  Within the bar: terms and atom_terms (fixed point, units of 2^-32): 4 units
    under exact transforms, ``GEOMETRIC`` x the input rounding as a score under rotations and translations (the restatement's
    largest deviation there: 1.5e-4 at shift_300, case 'own_targets', against 2.4e-4)."""
    name = 'dl_interaction_scores'
    SEEDS = {'own_targets': 371, 'shared_257': 372}

    def make(self, seed, own=True, shared=False):
        case = row_batch(seed, n_pocket=10 if own else 0)
        if shared:
            case['protein_x'], case['protein_type'] = protein_257(seed + 1, np.array([20.0, 20.0, 20.0]))
        return case

    def cases(self):
        kinds = {'own_targets': (True, False), 'shared_257': (False, True)}
        return {name: fixed_case(self, name, lambda s, k=k: self.make(s, *k)) for name, k in kinds.items()}

    def build(self, case, T):
        inputs = build_rows(case, T)
        inputs['xs_type'], _ = ir.interaction_types(inputs['x'], inputs['one_hot'], inputs['group'], InteractionTypes.table())
        if 'protein_x' in inputs:
            flags = np.array([ir.flags_of(t, 2, True, 0.0) for t in inputs['protein_type']], dtype=np.int64)
            inputs['protein_xs'] = flags
        return inputs

    def margins(self, inputs, run=None):
        from difflinker_amd.const import XS_RADII
        out, radius = InteractionTypes().margins(inputs), np.array(XS_RADII)      # the typing is done in the frame of the inputs
        for b in range(len(inputs['qm'])):
            rows, d, types = pair_distances(inputs, b)
            if d.size:
                s = d - (radius[inputs['types'][b, rows]][:, None] + radius[types][None, :])
                out.append((('cut', b), float(np.abs(d - 8.0).min())))
                out.append((('hydrophobic count', b), float(np.abs(s - 1.5).min())))
                out.append((('hbond count', b), float(np.abs(s).min())))
        return out

    def reference(self, inputs, run=None):
        from difflinker_amd.const import XS_RADII
        return ir.interaction_scores(inputs['x'], inputs['xs_type'], inputs['qm'], np.array(XS_RADII), inputs['tm'],
                                     inputs.get('protein_x'), inputs.get('protein_xs'))

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        for name in ('n_query', 'n_target', 'n_pairs', 'n_hbonds', 'n_hydrophobic', 'status'):
            same(out0[name], out1[name], name)
        worst = 0
        for b, sigma in enumerate(in1['sigma']):
            if T.exact:
                limit = ULPS                         # units of 2^-32: the output's own step
            else:
                limit = int(math.ceil(GEOMETRIC * input_rounding(in0['x'][b], in1['x'][b], in0.get('protein_x', np.zeros(1)),
                                                                 in1.get('protein_x', np.zeros(1))) * ir.ONE))
            diff = np.abs(out0['terms'][b] - out1['terms'][b]).max()
            atom = np.abs(out0['atom_terms'][b] - out1['atom_terms'][b][sigma]).max()
            assert diff <= limit and atom <= limit, ('terms', b, int(diff), int(atom), limit)
            worst = max(worst, int(diff), int(atom))
        return worst


# ---- dl_pharmacophore_features and dl_feature_match -----------------------------------------------------------------------------
class Pharmacophore(Entry):
    """Transforms: all (the families are read from the bond graph; the frame enters through the positions).  Exact: n_features,
    family_count, status, and the list as a multiset of (family, anchor, marked) - the anchor of a ring feature, "the ring's
    smallest atom", left out under a renumbering.  Within the bar: position after the inverse motion, matched by record."""
    name = 'dl_pharmacophore_features'
    FCAP = 24

    SEEDS = {'examples_a': 1, 'examples_b': 2, 'axes': 3}     # of the coordinates and marks; no rule here reads a distance

    @staticmethod
    def molecule(name, points, rng):
        symbols, bonds, _ = ph.EXAMPLES[name]
        n = len(symbols)
        return dict(molecule_of([ph.TYPE[s] for s in symbols], points, [], marked=[k for k in range(n) if rng.random() < 0.6]),
                    entries=[tuple(e) for e in bonds], aromatic=[e for e, bond in enumerate(bonds) if bond[3]])

    def cases(self):
        """The hand molecules of ``pharmacophore_ref.EXAMPLES`` on random coordinates around (20, 20, 20), in two batches, and
        'axes': rings as regular polygons in the xy plane around the origin (their centroids, the ring features' positions, are
        sums that cancel), a substituent on the x axis, an amine with its carbons on the three axes, an acid along z."""
        names = sorted(ph.EXAMPLES)
        out = {}
        for label, chosen in (('examples_a', names[:7]), ('examples_b', names[7:])):
            rng = np.random.default_rng(self.SEEDS[label])
            molecules = [self.molecule(name, 20.0 + rng.normal(0, 2, (len(ph.EXAMPLES[name][0]), 3)), rng) for name in chosen]
            out[label] = dict(molecules=molecules, width=13, pack_seed=self.SEEDS[label])
        rng = np.random.default_rng(self.SEEDS['axes'])
        hexagon, pentagon = pr.polygon(6, 1.39), pr.polygon(5, 1.38)
        out['axes'] = dict(molecules=[
            self.molecule('benzene', hexagon, rng), self.molecule('pyridine', hexagon, rng), self.molecule('pyrrole', pentagon, rng),
            self.molecule('furan', pentagon, rng), self.molecule('chlorobenzene', hexagon + [(hexagon[0][0] + 1.74, 0.0, 0.0)], rng),
            self.molecule('trimethylamine', [(0, 0, 0), (1.47, 0, 0), (0, 1.47, 0), (0, 0, 1.47)], rng),
            self.molecule('acetic acid', [(0, 0, 0), (0, 0, 1.5), (0, 0, 2.7), (0, 0, -1.3)], rng)], width=9, pack_seed=self.SEEDS['axes'])
        return out

    def build(self, case, T):
        return build_molecules(case, T, nf=NF9)

    def reference(self, inputs, run=None):
        return ph.batch_features(inputs, self.FCAP, None, inputs['mark'])

    def records(self, inputs, out, b, sigma, T):
        n = int(out['n_features'][b])
        inverse = np.argsort(sigma)
        rows = []
        for f in range(min(n, self.FCAP)):
            fam = int(out['family'][b, f])
            ring = fam in (ph.AROMATIC, ph.LUMPED)
            anchor = -1 if ring and T.kind == 'renumber' else int(inverse[out['anchor'][b, f]])
            rows.append(((fam, anchor, int(out['marked'][b, f])), out['position'][b, f].astype(np.float64)))
        return rows

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        for name in ('n_features', 'family_count', 'status'):
            same(out0[name], out1[name], name)
        worst = 0.0
        for b, sigma in enumerate(in1['sigma']):
            r0 = self.records(in0, out0, b, np.arange(len(sigma)), IDENTITY if T.kind != 'renumber' else T)
            r1 = self.records(in1, out1, b, sigma, T)
            key = lambda r: (r[0], tuple(np.round(r[1], 3)))            # noqa: E731
            r0 = sorted(r0, key=key)
            r1 = sorted([(k, T.undo(p)) for k, p in r1], key=key)
            assert [k for k, _ in r0] == [k for k, _ in r1], ('records', b)
            if r0:
                p0, p1 = np.stack([p for _, p in r0]), np.stack([p for _, p in r1])
                limit = bar(T, np.float32, out0['position'][b], in0['x'][b, in0['rows'][b]], in1['x'][b, in1['rows'][b]])
                worst = max(worst, close(p0, p1, limit, ('position', b)))
        return worst


class FeatureMatch(Entry):
    """Transforms: all, on both feature lists at once; a renumbering permutes the two lists independently.  Exact: n_a, n_b,
    n_matched, best_index (renamed).  Within the bar, as a distance: best_d2."""
    name = 'dl_feature_match'
    SEEDS = {'random': 581, 'sparse': 382}
    START = {'random': 381}
    RADIUS2 = 6.25

    def make(self, seed, B=6, Fa=14, Fb=11, box=5.0):
        rng = np.random.default_rng(seed)
        side = lambda F: dict(family=rng.integers(0, 4, (B, F)).astype(np.int32), position=f32(20.0 + rng.uniform(0, box, (B, F, 3))),   # noqa: E731
                              marked=rng.integers(0, 2, (B, F)).astype(np.int32), n_features=rng.integers(F - 4, F + 1, B).astype(np.int32))
        return dict(a=side(Fa), b=side(Fb))

    def cases(self):
        return {'random': fixed_case(self, 'random', self.make),
                'sparse': fixed_case(self, 'sparse', lambda s: self.make(s, B=16, Fa=5, Fb=6, box=3.0))}

    def build(self, case, T):
        out = {}
        for salt, side in enumerate('ab'):
            lists = case[side]
            B, F = lists['family'].shape
            new = {k: np.array(v) for k, v in lists.items()}
            new['position'] = T.apply(lists['position']).astype(np.float32)
            sigmas = []
            for b in range(B):
                n = int(lists['n_features'][b])
                sigma = np.concatenate([T.sigma(n, b, salt=salt + 2), np.arange(n, F)])
                sigmas.append(sigma)
                for name in ('family', 'position', 'marked'):
                    moved_rows = np.empty_like(new[name][b])
                    moved_rows[sigma] = new[name][b]
                    new[name][b] = moved_rows
            out[side] = new
            out['sigma_' + side] = sigmas
        out['sigma'] = out['sigma_b']
        return out

    def candidates(self, inputs, b):
        a, c = inputs['a'], inputs['b']
        na, nb = int(a['n_features'][b]), int(c['n_features'][b])
        d = np.sqrt(((a['position'][b, :na].astype(np.float64)[:, None] - c['position'][b, :nb].astype(np.float64)[None]) ** 2).sum(-1))
        return np.where(a['family'][b, :na][:, None] == c['family'][b, :nb][None, :], d, np.inf)

    def margins(self, inputs, run=None):
        out = []
        for b in range(len(inputs['a']['family'])):
            d = self.candidates(inputs, b)
            finite = d[np.isfinite(d)]
            if finite.size:
                out.append((('radius', b), float(np.abs(finite - math.sqrt(self.RADIUS2)).min())))
            for j in range(d.shape[1]):
                col = np.sort(d[:, j][np.isfinite(d[:, j])])
                if len(col) > 1:
                    out.append((('tie', b, j), float(col[1] - col[0])))
        return out

    def reference(self, inputs, run=None):
        a, b = inputs['a'], inputs['b']
        names = ('family', 'position', 'marked', 'n_features')
        return ph.feature_match(*(a[k] for k in names), *(b[k] for k in names), self.RADIUS2, False)

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        for name in ('n_a', 'n_b', 'n_matched'):
            same(out0[name], out1[name], name)
        worst = 0.0
        for b in range(len(out0['n_a'])):
            sa, sb = in1['sigma_a'][b], in1['sigma_b'][b]
            index1 = out1['best_index'][b][sb]
            index1 = np.where(index1 >= 0, np.argsort(sa)[np.maximum(index1, 0)], -1)
            same(out0['best_index'][b], index1, ('best_index', b))
            d0, d1 = np.sqrt(out0['best_d2'][b].astype(np.float64)), np.sqrt(out1['best_d2'][b][sb].astype(np.float64))
            limit = bar(T, np.float32, d0[np.isfinite(d0)], in0['a']['position'][b], in1['a']['position'][b])
            worst = max(worst, close(d0, d1, limit, ('best distance', b)))
        return worst


# ---- dl_shape_scores ------------------------------------------------------------------------------------------------------------
class Shape(Entry):
    """Transforms: the 48 signed axis permutations, translations by multiples of the lattice spacing and renumberings - and
    nothing else.  ``dl_shape_scores`` counts the points of a cubic lattice that is FIXED in the frame of the coordinates
    (spacing 0.5 A): a rotation or a translation off the lattice changes which points an atom covers, and the header says so
    ("a shift below its spacing changes the counts").  The signed permutations and lattice translations map the lattice onto
    itself, and with coordinates on multiples of 2^-10 every squared distance is exact in fp32 in any order of its sum: equality
    is exact.  Exact: all nine outputs.  No random rotation, no clearance: nothing is rounded."""
    name = 'dl_shape_scores'
    transforms = PERMS + MIRRORS + LATTICE_SHIFTS + RENUMBERINGS
    GRID = 2.0 ** -10

    def make(self, seed, B=6, na=12, nb=14, box=5.0):
        rng = np.random.default_rng(seed)
        case = dict(xa=[], xb=[], ta=[], tb=[])
        for b in range(B):
            centre = rng.integers(-40, 41, size=3) * 0.5
            for key, n in (('a', na - b % 3), ('b', nb - b % 4)):
                x = centre + np.round(rng.uniform(0, box, (n, 3)) / self.GRID) * self.GRID
                kind = rng.integers(0, 4, n)
                x[kind == 0] = np.round(x[kind == 0] * 2) / 2           # on lattice points
                x[kind == 1] = np.round(x[kind == 1] * 2) / 2 + 0.25    # on half spacings
                case['x' + key].append(x)
                case['t' + key].append(rng.integers(0, NF9, n))
        return case

    def cases(self):
        axes = dict(xa=[m['points'] for m in axis_molecules()[:3]], xb=[m['points'] + 0.25 for m in axis_molecules()[:3]],
                    ta=[np.asarray(m['types']) for m in axis_molecules()[:3]], tb=[np.asarray(m['types']) for m in axis_molecules()[:3]])
        for key in ('xa', 'xb'):
            axes[key] = [np.round(x / self.GRID) * self.GRID for x in axes[key]]
        return {'clouds': self.make(391), 'small': self.make(392, B=12, na=4, nb=3, box=2.0), 'axes': axes}

    def build(self, case, T):
        B = len(case['xa'])
        widths = {'a': max(len(x) for x in case['xa']) + 3, 'b': max(len(x) for x in case['xb']) + 2}
        rng = np.random.default_rng(17 + (T.seed or 0))
        out = {}
        for salt, key in enumerate('ab'):
            W = widths[key]
            x = rng.choice(np.float32([1e4, -3e7, 0.125]), size=(B, W, 3))
            one_hot = rng.uniform(-5, 5, size=(B, W, NF9)).astype(np.float32)
            mask = np.zeros((B, W), np.float32)
            for b in range(B):
                n = len(case['x' + key][b])
                rows = np.sort(rng.choice(W, n, replace=False))
                order = np.argsort(T.sigma(n, b, salt=salt))
                points = T.apply(case['x' + key][b])
                assert np.array_equal(points.astype(np.float32).astype(np.float64), points), 'the transform is exact'
                x[b, rows], one_hot[b, rows], mask[b, rows] = points[order], np.eye(NF9, dtype=np.float32)[case['t' + key][b][order]], 1
            out.update({'x_' + key: x, 'one_hot_' + key: one_hot, 'mask_' + key: mask})
        out['sigma'] = [np.arange(0)] * B
        return out

    @staticmethod
    def arrays(inputs):
        return tuple(inputs[k] for k in ('x_a', 'one_hot_a', 'mask_a', 'x_b', 'one_hot_b', 'mask_b'))

    def reference(self, inputs, run=None):
        return shape_ref.shape_scores(*self.arrays(inputs))

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        for name in shape_ref.FIELDS:
            same(out0[name], out1[name], name)
        assert not np.asarray(out0['status']).any() and np.asarray(out0['vol_min']).sum() > 0, 'the pairs overlap and are scored'


# ---- dl_best_rmsd ---------------------------------------------------------------------------------------------------------------
class Rmsd(Entry):
    """Transforms: all, applied to the pair as a whole (a mirror of BOTH molecules keeps the RMSD; of one it does not); the
    second molecule of every pair already sits in a frame of its own (a seeded rotation and 75 A away).  A renumbering permutes the atoms of the two
    molecules independently and renames the maps, which keep their order in the table.  Exact: best (the maps' values differ
    by ``MARGIN`` or more), status.  Within the bar: rmsd."""
    name = 'dl_best_rmsd'
    SEEDS = {'tables': 401, 'ring': 402}

    def make(self, seed, ring=False):
        rng = np.random.default_rng(seed)
        pairs = []
        for n, size in ((7, 1), (7, 12), (5, 3), (9, 65), (1, 1), (2, 2), (3, 4), (12, 7)):
            if ring:
                n, size = 6, 12
                angle = np.arange(6) * np.pi / 3
                a = np.stack([1.39 * np.cos(angle), 1.39 * np.sin(angle), np.zeros(6)], 1) + rng.normal(0, 0.05, (6, 3))
                maps = [[(s * k + r) % 6 for k in range(6)] for s in (1, -1) for r in range(6)]
                b = a[np.argsort(maps[int(rng.integers(12))])] + rng.normal(0, 0.25, (6, 3))
            else:
                a = 2.0 * rng.normal(size=(n, 3))
                true = rng.permutation(n)
                b = np.empty((n, 3))
                b[true] = a + rng.normal(0, 0.2, (n, 3))
                maps = [rng.permutation(n).tolist() for _ in range(size - 1)]
                maps.insert(int(rng.integers(size)), true.tolist())
                maps = [m for k, m in enumerate(maps) if m not in maps[:k]]
            pairs.append(dict(a=f32(a + 30.0), b=f32(b @ rotation(seed + n).T - 45.0), maps=maps))
        return dict(pairs=pairs)

    def cases(self):
        return {'tables': fixed_case(self, 'tables', self.make),
                'ring': fixed_case(self, 'ring', lambda s: self.make(s, ring=True))}

    def build(self, case, T):
        pairs, sigmas = [], []
        for p, pair in enumerate(case['pairs']):
            n = len(pair['a'])
            sa, sb = T.sigma(n, p, salt=1), T.sigma(n, p, salt=2)
            a, b = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
            a[sa], b[sb] = T.apply(pair['a']).astype(np.float32), T.apply(pair['b']).astype(np.float32)
            maps = []
            for image in pair['maps']:
                new = [0] * n
                for k in range(n):
                    new[sa[k]] = int(sb[image[k]])
                maps.append(new)
            pairs.append(dict(a=a, b=b, maps=maps))
            sigmas.append(sa)
        return dict(pairs=pairs, sigma=sigmas)

    def values(self, inputs):
        return [[rmsd_ref.kabsch_rmsd(pair['a'], np.asarray(pair['b'], dtype=np.float64)[list(image)]) for image in pair['maps']]
                for pair in inputs['pairs']]

    def margins(self, inputs, run=None):
        out = []
        for p, values in enumerate(self.values(inputs)):
            ordered = sorted(values)
            if len(ordered) > 1:
                out.append((('best against the next map', p), ordered[1] - ordered[0]))
        return out

    def reference(self, inputs, run=None):
        found = [rmsd_ref.best_rmsd(pair['a'], pair['b'], pair['maps']) for pair in inputs['pairs']]
        return dict(rmsd=np.array([v for v, _ in found]), best=np.array([k for _, k in found], np.int32), status=np.zeros(len(found), np.int32))

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        same(out0['best'], out1['best'], 'best')
        same(out0['status'], out1['status'], 'status')
        worst = 0.0
        for p, (pair0, pair1) in enumerate(zip(in0['pairs'], in1['pairs'])):
            limit = bar(T, np.float32, [out0['rmsd'][p]], pair0['a'], pair0['b'], pair1['a'], pair1['b'])
            worst = max(worst, close(out0['rmsd'][p], out1['rmsd'][p], limit, ('rmsd', p)))
        return worst


# ---- dl_pocket_select -----------------------------------------------------------------------------------------------------------
class Pocket(Entry):
    """Transforms: all, applied to every protein and every ligand alike; a renumbering permutes the atoms of each protein
    among themselves (their groups go along) and scatters the ligand rows anew.  Exact: all seven outputs - ``member`` by
    protein atom, ``index`` as the set of atoms it names.  No continuous output."""
    name = 'dl_pocket_select'
    SEEDS = {'two_proteins': 411, 'protein_257': 412}

    def make(self, seed, sizes=(60, 31), pairs=6):
        rng = np.random.default_rng(seed)
        proteins = []
        for m in sizes:
            x, group, g = [], [], 0
            while len(x) < m:
                middle = rng.uniform(-9.0, 9.0, 3)
                for _ in range(min(int(rng.integers(1, 9)), m - len(x))):
                    x.append(middle + rng.normal(0, 1.5, 3))
                    group.append(g)
                g += 1
            proteins.append((f32(np.array(x) + 25.0), np.array(group, np.int32)))
        ligands = [(p % len(sizes), np.round(25.0 + rng.normal(0, 2.0, (int(rng.integers(1, 12)), 3)), 4)) for p in range(pairs)]
        return dict(proteins=proteins, ligands=ligands, width=14)

    def cases(self):
        return {'two_proteins': fixed_case(self, 'two_proteins', self.make),
                'protein_257': fixed_case(self, 'protein_257', lambda s: self.make(s, sizes=(257,), pairs=4))}

    def build(self, case, T):
        rng = np.random.default_rng(23 + (T.seed or 0))
        taus = [T.sigma(len(g), p, salt=3) for p, (_, g) in enumerate(case['proteins'])]
        xs, groups = [], []
        for (x, g), tau in zip(case['proteins'], taus):
            moved_x, moved_g = np.empty((len(g), 3), np.float32), np.empty(len(g), np.int32)
            moved_x[tau], moved_g[tau] = T.apply(x).astype(np.float32), g
            xs.append(moved_x)
            groups.append(moved_g)
        B, W = len(case['ligands']), case['width']
        out = dict(protein_x=np.concatenate(xs), protein_group=np.concatenate(groups),
                   protein_offset=np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32),
                   pair_protein=np.array([p for p, _ in case['ligands']], np.int32),
                   ligand_x=rng.choice(np.array([np.nan, np.inf, -1e300]), (B, W, 3)), ligand_mask=np.zeros((B, W), np.float32),
                   taus=taus, sigma=[np.arange(0)] * B)
        for b, (_, lig) in enumerate(case['ligands']):
            rows = np.sort(rng.choice(W, len(lig), replace=False))
            out['ligand_x'][b, rows] = T.apply(lig)[np.argsort(T.sigma(len(lig), b, salt=4))]      # fp64: the entry point reads doubles
            out['ligand_mask'][b, rows] = 1
        return out

    R = 300

    def margins(self, inputs, run=None):
        out = []
        for b, p in enumerate(inputs['pair_protein']):
            lo, hi = inputs['protein_offset'][p], inputs['protein_offset'][p + 1]
            xp = inputs['protein_x'][lo:hi].astype(np.float64)
            xl = inputs['ligand_x'][b][inputs['ligand_mask'][b] != 0]
            out.append((('cut-off', b), float(np.abs(np.sqrt(((xp[:, None] - xl[None]) ** 2).sum(-1)) - 6.0).min())))
        return out

    def reference(self, inputs, run=None):
        return pocket_ref.select_pockets(inputs['protein_x'], inputs['protein_group'], inputs['protein_offset'], inputs['pair_protein'],
                                         inputs['ligand_x'], inputs['ligand_mask'], 6.0, None, self.R)

    def compare(self, case, T, in0, out0, in1, out1, run=None):
        for name in ('n_ligand', 'n_contact_atoms', 'n_groups_selected', 'n_pocket', 'status'):
            same(out0[name], out1[name], name)
        assert int(out0['n_pocket'].min()) >= 0 and int(out0['n_contact_atoms'].sum()) > 0
        for b, p in enumerate(in0['pair_protein']):
            tau = in1['taus'][p]
            same(out0['member'][b, :len(tau)], out1['member'][b, :len(tau)][tau], ('member', b))
            named = lambda out: out['index'][b][out['index'][b] >= 0]       # noqa: E731
            assert sorted(named(out0).tolist()) == sorted(np.argsort(tau)[named(out1)].tolist()), ('index', b)
            assert np.all(np.diff(named(out1)) > 0), ('index ascends', b)


# ---- the wrapper chains: perceive_bonds -> refine_bond_orders -> add_hydrogens / pose_checks / relax ------------------------------
def chain_molecules(seed):
    """Molecules whose bonds the distance table finds: ring edges of 1.40 A (a single bond for every pair of C, N and O, clear
    of the double bond's bound), substituents at 1.50 A, chains of 1.54 A, every atom displaced by N(0, 0.02 A).  Linker atoms
    are marked."""
    rng = np.random.default_rng(seed)
    C, N_, O = pr.C, pr.N_, pr.O
    hexagon, pentagon = pr.polygon(6, 1.40), pr.polygon(5, 1.40)
    sub = lambda ring, k, length=1.50: tuple(np.asarray(ring[k]) * (1.0 + length / np.linalg.norm(ring[k])))      # noqa: E731
    built = [([C] * 7, hexagon + [sub(hexagon, 0)]), ([N_] + [C] * 6, hexagon + [sub(hexagon, 3)]),
             ([N_, C, C, C, C, C], pentagon + [sub(pentagon, 2)]), ([O, C, C, C, C], pentagon),
             ([C] * 6, pr.zigzag(6)), ([C, C, O, C, N_], pr.zigzag(5, 1.47)),
             ([C] * 8, hexagon + [sub(hexagon, 0), sub(hexagon, 0, 3.0)])]
    out = []
    for types, points in built:
        n = len(types)
        points = np.asarray(points, dtype=np.float64) + rng.normal(0, 0.02, (n, 3)) + 20.0
        out.append(molecule_of(types, points, marked=[k for k in range(n) if k % 3 != 1]))
    return dict(molecules=out, width=11, pack_seed=seed)


def chain_reference(inputs):
    """``perceive_bonds`` and ``refine_bond_orders`` restated: the inputs with the list, its Kekule orders, ``planar`` =
    atom_aromatic, ``bond_aromatic`` and the status of the two launches filled in (capacity 4 N, as the wrappers choose)."""
    B, N = inputs['mask'].shape
    out = dict(inputs, bonds=np.zeros((B, 4 * N, 3), np.int32), n_in=np.zeros(B, np.int32))
    for b in range(B):
        _, types, points = real_molecule(inputs, b)
        found = pr.perceive(types.tolist(), points)
        out['bonds'][b, :len(found)] = np.asarray(found, np.int32).reshape(len(found), 3)
        out['n_in'][b] = len(found)
    arom = ar.aromatic_rings(inputs['x'], inputs['one_hot'], inputs['mask'], out['bonds'], out['n_in'], ar.ring_class_table(hr.ATOM2IDX),
                             np.zeros(B, np.int32), inputs['drop'], inputs['mark'])
    out['bonds'][:, :, 2] = arom['order_out']
    out.update(planar=arom['atom_aromatic'], bond_aromatic=arom['bond_aromatic'], status=arom['status'], n_aromatic_rings=arom['n_aromatic_rings'])
    out.update(atom_planar=out['planar'], n_bonds_in=out['n_in'], status_in=out['status'])
    return out


class Chain:
    """A wrapper chain as an entry point: ``reference`` (and the GPU implementation) first derive the list, and write what
    they derived into ``inputs`` for ``compare`` to read.  One case, a subset of the transforms of every kind."""
    transforms = PERMS[1:4] + MIRRORS[:3] + ROTATIONS + SHIFTS + RENUMBERINGS
    SEEDS = {'rings_and_chains': 421}

    def cases(self):
        return {'rings_and_chains': chain_molecules(self.SEEDS['rings_and_chains'])}

    def margins(self, inputs, run=None):
        derived = chain_reference(inputs)
        return Bonds().margins(inputs) + Aromatic().margins(derived) + super().margins(derived, run)

    def reference(self, inputs, run=None):
        derived = chain_reference(inputs)
        inputs.update({k: derived[k] for k in ('bonds', 'n_in', 'planar', 'bond_aromatic', 'status', 'atom_planar', 'n_bonds_in', 'status_in')})
        out = super().reference(inputs, run)
        out['chain_bonds'] = [sorted((min(i, j), max(i, j)) for i, j, _ in inputs['bonds'][b, :inputs['n_in'][b]].tolist())
                              for b in range(len(inputs['n_in']))]
        out['n_aromatic_rings'] = derived['n_aromatic_rings']
        return out

    def compare(self, case, T, in0, out0, in1, out1, run=None, **kw):
        same(out0['n_aromatic_rings'], out1['n_aromatic_rings'], 'n_aromatic_rings')
        assert int(np.sum(out0['n_aromatic_rings'])) >= 4, 'the rings are found'
        for b, sigma in enumerate(in1['sigma']):
            back = sorted(tuple(sorted(p)) for p in renamed_back(out1['chain_bonds'][b], sigma))
            assert out0['chain_bonds'][b] == back, ('the intermediate bond list', b)
        return super().compare(case, T, in0, out0, in1, out1, run, **kw)


class ChainHydrogens(Chain, Hydrogens):
    """``perceive_bonds`` -> ``refine_bond_orders`` -> ``add_hydrogens``: compared as ``dl_add_hydrogens``."""
    name = 'chain:add_hydrogens'


class ChainPoseChecks(Chain, PoseChecks):
    """``analyze_pose_checks``: compared as ``dl_pose_checks``."""
    name = 'chain:analyze_pose_checks'


class ChainRelax(Chain, Relax):
    """``relax_samples`` at 1 step: compared as ``dl_relax_molecules`` with the bar of that entry point at 1 step."""
    name = 'chain:relax_samples'
    runs = (1,)

    def runs_of(self, case_name):
        return self.runs


CHAINS = [ChainHydrogens(), ChainPoseChecks(), ChainRelax()]
ENTRIES = [Bonds(), Aromatic(), Hydrogens(), PoseChecks(), Clash(), InteractionTypes(), InteractionScores(), Pharmacophore(),
           FeatureMatch(), Shape(), Rmsd(), Relax(), Pocket()]
ENTRY_POINTS = {e.name: e for e in ENTRIES + CHAINS}


def parameters(entries=None):
    """``(entry name, case name, transform name, run)`` of every check."""
    out = []
    for e in ENTRIES if entries is None else entries:
        for case_name in e.case_names():
            for T in e.transforms_of(case_name):
                for run in e.runs_of(case_name):
                    out.append((e.name, case_name, T.name, run))
    return out


def compare(entry, case_name, T, in0, out0, in1, out1, run=None):
    e = ENTRY_POINTS[entry] if isinstance(entry, str) else entry
    kwargs = dict(case_name=case_name) if isinstance(e, Hydrogens) else {}
    assert out0 is not out1 and in0 is not in1
    return e.compare(e.case(case_name), T, in0, out0, in1, out1, run, **kwargs)


def check(implementation, entry, case_name, transform, run=None, cache=None):
    """One check: ``implementation(entry object, inputs, run)`` on the base case (kept in ``cache`` by entry, case and run) and
    on the transformed case, compared after ``undo``.  Returns what ``compare`` measured."""
    e, T = ENTRY_POINTS[entry], TRANSFORMS[transform]
    cache = {} if cache is None else cache
    key = (entry, case_name, run)
    if key not in cache:
        inputs = e.build(e.case(case_name), IDENTITY)
        cache[key] = (inputs, implementation(e, inputs, run))
    in0, out0 = cache[key]
    in1 = e.build(e.case(case_name), T)
    return compare(e, case_name, T, in0, out0, in1, implementation(e, in1, run), run)
