"""Bond perception of sampled batches — the reference's ``src/molecule_builder.py`` (``build_xae_molecule``,
``get_bond_order``) for a whole batch in one HIP launch (``csrc/bonds.hip``), on the tensors ``sample_chain`` left on the
device, plus the connectivity check of ``metrics.is_connected``.

Atoms are numbered the way the reference numbers them: the rows with ``node_mask != 0`` in row order (it masks a molecule
before it builds it), so atom ``k`` of ``bonds``, ``valence`` and ``component`` is the ``k``-th line of the ``.xyz`` / ``.sdf``
file of the same molecule.  RDKit objects are not built: ``build_xae_molecules`` stops at the reference's ``(X, A, E)``
triple, and validity is reported as numbers (valences, component counts), never as RDKit's sanitisation.
"""
from collections import namedtuple

import torch

from . import _lib, const

Bonds = namedtuple('Bonds', 'n_bonds bonds valence n_components component status')
Aromatic = namedtuple('Aromatic', 'bond_aromatic atom_aromatic n_planar_rings n_aromatic_rings n_aromatic_marked status')
Hydrogens = namedtuple('Hydrogens', 'n_h h_count parent x status')

_TABLES = {}
_RING_CLASSES = {}
_HYDROGEN_TABLES = {}
Relaxed = namedtuple('Relaxed', 'x energy steps_done f_max moved2 status')
_RELAX_TABLES = {}


def _table(device, is_geom, margins):
    key = (device, bool(is_geom), tuple(float(m) for m in margins))
    if key not in _TABLES:
        _TABLES[key] = const.bond_threshold_table(is_geom, margins).to(device).contiguous()
    return _TABLES[key]


def perceive_bonds(one_hot, x, node_mask, is_geom, margins=const.MARGINS_EDM, capacity=None):
    """Bonds of every molecule of a batch: ``one_hot [B,N,nf]``, ``x [B,N,3]`` (Angstrom), ``node_mask [B,N,1]`` or ``[B,N]``
    on the HIP device.  Returns device int32 tensors, without a host synchronisation:

    ``n_bonds [B]``; ``bonds [B,capacity,3]`` rows ``(i, j, order)`` with ``j < i`` in row-major order of ``(i, j)``, valid up
    to ``n_bonds``; ``valence [B,N]``; ``n_components [B]``; ``component [B,N]`` (smallest atom index of the atom's component,
    -1 beyond the atom count); ``status [B]`` (``_lib.DL_BONDS_OVERFLOW``: more bonds than ``capacity``, ``n_bonds`` is
    still the true count; ``_lib.DL_BONDS_NONFINITE``: a NaN / inf coordinate, which bonds to nothing).
    ``capacity`` defaults to ``4 * N`` bonds per molecule (a valid heavy-atom graph has at most ``2 * N``)."""
    _lib.require_device('perceive_bonds', one_hot=one_hot, x=x, node_mask=node_mask)
    B, N, nf = one_hot.shape
    if x.shape != (B, N, 3) or node_mask.numel() != B * N:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, x {tuple(x.shape)}, '
                         f'node_mask {tuple(node_mask.shape)}')
    dev = one_hot.device
    one_hot, x, node_mask = (_lib.dense(t, dev, torch.float32) for t in (one_hot, x, node_mask))
    table = _table(dev, is_geom, margins)
    capacity = 4 * N if capacity is None else int(capacity)
    out = Bonds(*(_lib.empty_i32(dev, *shape) for shape in ((B,), (B, capacity, 3), (B, N), (B,), (B, N), (B,))))
    args = _lib.DLBondsArgs(B=B, N=N, nf=nf, one_hot=one_hot.data_ptr(), x=x.data_ptr(), node_mask=node_mask.data_ptr(),
                            table=table.data_ptr(), table_len=table.numel(), capacity=capacity,
                            n_bonds=out.n_bonds.data_ptr(), bonds=out.bonds.data_ptr() if capacity else None,
                            valence=out.valence.data_ptr(), n_components=out.n_components.data_ptr(),
                            component=out.component.data_ptr(), status=out.status.data_ptr(), workspace=None,
                            workspace_bytes=0)
    _lib.launch('dl_perceive_bonds', args, dev)
    return out


def perceive_all_bonds(one_hot, x, node_mask, is_geom, margins=const.MARGINS_EDM):
    """``perceive_bonds`` whose list holds every bond of every molecule: when the default capacity overflows (atoms piled
    on one another, as an untrained model places them) the launch is repeated with the largest ``n_bonds`` as capacity.
    Reads ``n_bonds`` on the host, so it synchronises; the writers and ``build_xae_molecules`` go through it."""
    found = perceive_bonds(one_hot, x, node_mask, is_geom, margins)
    most = int(found.n_bonds.max()) if found.n_bonds.numel() else 0
    if most > found.bonds.shape[1]:
        found = perceive_bonds(one_hot, x, node_mask, is_geom, margins, capacity=most)
    return found


_KERNEL_READS = ('n_bonds', 'bonds', 'valence', 'n_components', 'status')    # ``component`` goes to no kernel: left as it is


def _canonical_members(found, B, device):
    """``found`` with every member a kernel reads (``_KERNEL_READS``) that is not ``None`` as a dense int32 tensor on ``device``
    - the layout the kernels read at a member's ``data_ptr()``.  A member that is one already is passed on as it is (no copy).
    ``bonds`` must be ``[B,capacity,3]`` and every other such member must have ``B`` rows; ``ValueError`` names the member that
    is not."""
    if not torch.is_tensor(found.bonds) or found.bonds.dim() != 3 or found.bonds.shape[0] != B or found.bonds.shape[2] != 3:
        shape = tuple(found.bonds.shape) if torch.is_tensor(found.bonds) else None
        raise ValueError(f'shapes disagree: bonds {shape} of a Bonds for {B} molecules must be [{B},capacity,3]')
    new = {}
    for name in _KERNEL_READS:
        t = getattr(found, name)
        if t is None:
            continue
        if t.dim() < 1 or t.shape[0] != B:
            raise ValueError(f'shapes disagree: {name} {tuple(t.shape)} of a Bonds for {B} molecules')
        new[name] = t.to(device=device, dtype=torch.int32).contiguous()
    return found._replace(**new)


def normalize_bonds(found, B, device, who):
    """The ``Bonds`` a wrapper hands to a kernel: ``found`` may be the caller's own - the list int64 (``torch.tensor(rows)``) or a
    capacity slice ``wider[:, :capacity]`` of a longer one, the counts any integer dtype, strided or sliced - and every member
    the kernel reads becomes dense int32 (``_canonical_members``; a ``Bonds`` of ``perceive_bonds`` is not copied).  Members on
    the host raise ``HipLibraryError``: there is no CPU fallback."""
    _lib.require_device(who, **{name: getattr(found, name) for name in _KERNEL_READS})
    return _canonical_members(found, B, device)


def _ring_classes(device, is_geom):
    key = (device, bool(is_geom))
    if key not in _RING_CLASSES:
        _RING_CLASSES[key] = const.ring_class_table(is_geom).to(device).contiguous()
    return _RING_CLASSES[key]


def refine_bond_orders(found, one_hot, x, node_mask, is_geom, drop_mask=None, mark_mask=None, planarity=0.1,
                       substituent=0.5):
    """Kekule bond orders for the planar five- and six-rings of every molecule, from the 3D geometry, and the aromatic rings
    among them (``dl_aromatic_rings``, ``csrc/aromatic.hip``): ONE launch on the result ``found`` of ``perceive_bonds`` for
    the same ``one_hot``, ``x`` and ``node_mask``, without a host synchronisation.  The distance table of ``perceive_bonds``
    turns an aromatic ring into an arbitrary mix of single and double bonds; this replaces the orders inside such rings and
    leaves every other order alone.

    THE RULE is this project's own (``include/difflinker_hip.h`` states it in full; ``tests/aromatic_ref.py`` restates it): it
    is NOT RDKit's aromaticity model and NOT OpenBabel's bond typing.  Ring atoms are C and N of degree 2 or 3 and O and S of
    degree 2; a chordless 5- or 6-cycle of them is planar when its atoms lie within ``planarity`` (A) and their other
    neighbours within ``substituent`` (A) of the plane through its centroid whose normal is the ring's area vector; connected
    planar rings form a system; O, S and three-bonded N give two electrons and take no ring double bond, an atom with a
    double bond out of the rings gives none, and a matching that covers the most carbons, then the most two-bonded N, then is
    lexicographically smallest, places the double bonds; a ring with six electrons and every carbon covered is aromatic.
    No hydrogens (N-H and =N- are told apart only by the matching), no charges, rings of 5 and 6 atoms only; a planar
    saturated ring is misread as conjugated.

    ``drop_mask`` (the pocket) removes atoms together with their bonds, ``mark_mask`` (the linker) marks atoms, both
    ``[B,N]`` or ``[B,N,1]`` by row.  Returns ``(refined, aromatic)``: ``refined`` is a ``Bonds`` whose list carries the new
    orders (1, 2 or 3, never 4; 0 for an entry that is no bond) and whose ``valence`` is their sum per atom - whatever takes a
    ``Bonds`` takes it; ``aromatic`` holds ``bond_aromatic [B,capacity]``, ``atom_aromatic [B,N]``, ``n_planar_rings``,
    ``n_aromatic_rings``, ``n_aromatic_marked`` (aromatic rings all of whose atoms are marked) and ``status`` ``[B]``: the bits
    of ``found.status`` plus ``_lib.DL_AROM_*`` (more than 256 kept atoms or 64 planar rings: the orders pass through; a
    system of more than 32 atoms keeps its orders)."""
    masks = (node_mask,) + tuple(m for m in (drop_mask, mark_mask) if m is not None)
    _lib.require_device('refine_bond_orders', one_hot=one_hot, x=x, bonds=found.bonds, node_mask=node_mask,
                        drop_mask=drop_mask, mark_mask=mark_mask)
    B, N, nf = one_hot.shape
    if x.shape != (B, N, 3) or any(m.numel() != B * N for m in masks) or found.bonds.dim() != 3 or found.bonds.shape[0] != B:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, x {tuple(x.shape)}, masks '
                         f'{[tuple(m.shape) for m in masks]}, bonds {tuple(found.bonds.shape)}')
    dev = one_hot.device
    given = normalize_bonds(found, B, dev, 'refine_bond_orders')
    one_hot, x, node_mask, drop_mask, mark_mask = (_lib.dense(t, dev, torch.float32)
                                                   for t in (one_hot, x, node_mask, drop_mask, mark_mask))
    classes = _ring_classes(dev, is_geom)
    if classes.numel() < nf:
        raise ValueError(f'one_hot has {nf} types, the vocabulary {classes.numel()}')
    capacity = given.bonds.shape[1]
    bonds = given.bonds
    order, valence = _lib.empty_i32(dev, B, capacity), _lib.empty_i32(dev, B, N)
    out = Aromatic(*(_lib.empty_i32(dev, *shape) for shape in ((B, capacity), (B, N), (B,), (B,), (B,), (B,))))
    args = _lib.DLAromaticArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(),
        drop_mask=_lib.ptr(drop_mask), mark_mask=_lib.ptr(mark_mask), ring_class=classes.data_ptr(), capacity=capacity, n_bonds_in=given.n_bonds.data_ptr(),
        bonds=bonds.data_ptr() if capacity else None, status_in=given.status.data_ptr(),
        tol2_ring=float(planarity) ** 2, tol2_sub=float(substituent) ** 2,
        order_out=order.data_ptr() if capacity else None, bond_aromatic=out.bond_aromatic.data_ptr() if capacity else None,
        atom_aromatic=out.atom_aromatic.data_ptr(), valence_out=valence.data_ptr(),
        n_planar_rings=out.n_planar_rings.data_ptr(), n_aromatic_rings=out.n_aromatic_rings.data_ptr(),
        n_aromatic_marked=out.n_aromatic_marked.data_ptr(), status=out.status.data_ptr())
    _lib.launch('dl_aromatic_rings', args, dev)
    refined = found._replace(bonds=torch.cat([bonds[:, :, :2], order[:, :, None]], dim=2), valence=valence)
    return refined, out


def _hydrogen_tables(device, is_geom):
    key = (device, bool(is_geom))
    if key not in _HYDROGEN_TABLES:
        _HYDROGEN_TABLES[key] = (const.default_valence_table(is_geom).to(device).contiguous(),
                                 const.xh_length_table(is_geom).to(device).contiguous())
    return _HYDROGEN_TABLES[key]


def add_hydrogens(found, one_hot, x, node_mask, is_geom, drop_mask=None, atom_planar=None, capacity=None):
    """Explicit hydrogens with 3D positions for every molecule of a batch (``dl_add_hydrogens``, ``csrc/hydrogens.hip``):
    ONE launch on the result ``found`` of ``perceive_bonds`` or ``refine_bond_orders`` for the same ``one_hot``, ``x`` and
    ``node_mask``, without a host synchronisation.

    THE RULE is this project's own (``include/difflinker_hip.h`` states it in full; ``tests/hydrogens_ref.py`` restates it): it
    is NOT RDKit's ``AddHs(addCoords=True)`` and NOT OpenBabel's.  An atom gets ``default valence - sum of its bond orders``
    hydrogens (``const.DEFAULT_VALENCE``; none when it is over-valent) at ``const.XH_LENGTH`` from it: linear with a triple or
    two double bonds, trigonal with one double bond (or with ``atom_planar`` set, two neighbours and one hydrogen: a pyrrole
    N-H), tetrahedral otherwise, staggered or trans to the neighbour's first other neighbour.  With the distance table's
    orders the counts inside aromatic rings are arbitrary: pass the ``refined`` list of ``refine_bond_orders`` and its
    ``atom_aromatic`` as ``atom_planar``.  An amide or aniline N comes out pyramidal; there are no charges, so a carboxylate
    is written as an acid and an ammonium as an amine; P and S above their default valence get none.

    ``drop_mask`` (the pocket) removes atoms together with their bonds, ``[B,N]`` or ``[B,N,1]`` by row; ``atom_planar`` is
    ``[B,N]`` by atom number.  Returns a ``Hydrogens`` of device tensors: ``n_h [B]`` (the true count), ``h_count [B,N]`` by
    atom number, ``parent [B,capacity]`` (atom numbers) and ``x [B,capacity,3]`` (fp64), valid up to ``n_h`` and zero beyond,
    and ``status [B]``: the bits of ``found.status`` plus ``_lib.DL_HYDRO_*`` (more than 256 kept atoms or a non-finite
    coordinate: no hydrogens; ``DL_HYDRO_OVERFLOW``: more than ``capacity``).  ``capacity`` defaults to ``4 * N``, which
    cannot overflow."""
    masks = (node_mask,) + ((drop_mask,) if drop_mask is not None else ())
    others = masks + ((atom_planar,) if atom_planar is not None else ())
    _lib.require_device('add_hydrogens', one_hot=one_hot, x=x, node_mask=node_mask, drop_mask=drop_mask,
                        atom_planar=atom_planar)
    B, N, nf = one_hot.shape
    if x.shape != (B, N, 3) or any(m.numel() != B * N for m in others):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, x {tuple(x.shape)}, masks '
                         f'{[tuple(m.shape) for m in others]}')
    dev = one_hot.device
    given = normalize_bonds(found, B, dev, 'add_hydrogens')
    one_hot, x, node_mask, drop_mask = (_lib.dense(t, dev, torch.float32) for t in (one_hot, x, node_mask, drop_mask))
    if atom_planar is not None:
        atom_planar = _lib.dense(atom_planar.reshape(B, N) != 0, dev, torch.int32)
    valence, length = _hydrogen_tables(dev, is_geom)
    if valence.numel() < nf:
        raise ValueError(f'one_hot has {nf} types, the vocabulary {valence.numel()}')
    capacity = 4 * N if capacity is None else int(capacity)
    bond_capacity = given.bonds.shape[1]
    out = Hydrogens(_lib.empty_i32(dev, B), _lib.empty_i32(dev, B, N), torch.zeros((B, capacity), dtype=torch.int32, device=dev),
                    torch.zeros((B, capacity, 3), dtype=torch.float64, device=dev), _lib.empty_i32(dev, B))
    args = _lib.DLHydrogensArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(),
        drop_mask=_lib.ptr(drop_mask), atom_planar=_lib.ptr(atom_planar), default_valence=valence.data_ptr(), xh_length=length.data_ptr(), capacity=bond_capacity,
        n_bonds_in=given.n_bonds.data_ptr(), bonds=given.bonds.data_ptr() if bond_capacity else None,
        status_in=_lib.ptr(given.status), Hcap=capacity, n_h=out.n_h.data_ptr(), h_count=out.h_count.data_ptr(),
        h_parent=out.parent.data_ptr() if capacity else None, h_x=out.x.data_ptr() if capacity else None,
        status=out.status.data_ptr())
    _lib.launch('dl_add_hydrogens', args, dev)
    return out


def _relax_tables(device, is_geom, reach_scale):
    key = (device, bool(is_geom), float(reach_scale))
    if key not in _RELAX_TABLES:
        _RELAX_TABLES[key] = tuple(t.to(device).contiguous() for t in (
            const.length0_table(is_geom), const.aromatic_length0_table(is_geom), const.ideal_cos_table(),
            const.relax_reach_table(is_geom, reach_scale)))
    return _RELAX_TABLES[key]


def relax(found, one_hot, x, node_mask, is_geom, mark_mask, drop_mask=None, atom_planar=None, bond_aromatic=None,
          use_wall=True, steps=const.RELAX_STEPS, reach_scale=const.RELAX_REACH_SCALE, **constants):
    """A restrained clean-up of the marked atoms of every molecule (``dl_relax_molecules``, ``csrc/relax.hip``): ONE launch on
    the result ``found`` of ``perceive_bonds`` or ``refine_bond_orders`` for the same ``one_hot``, ``x`` and ``node_mask``,
    without a host synchronisation.  Only the atoms of ``mark_mask`` (the linker; ``None``: every kept atom) move; every other
    row of ``x`` comes back bit for bit.

    THE RULE is this project's own (``include/difflinker_hip.h`` states it in full; ``tests/relax_ref.py`` restates it): it is
    NOT UFF, NOT MMFF and NOT RDKit's or OpenBabel's optimiser, and its energies are in units of its own.  ``steps`` steps of
    FIRE (Bitzek et al., PRL 97, 170201) in fp64 down the sum of: harmonic bonds to the typical length of their order
    (``const.BOND_LENGTHS``; ``const.AROMATIC_LENGTHS`` for the bonds ``bond_aromatic`` flags), harmonic terms in the cosine
    of the angles to the ideal of the centre's class (the classes of ``metrics.pose_checks``; three-, four- and five-ring
    angles exempt), a soft repulsion between atoms four or more bonds apart inside ``reach_scale`` times the sum of their
    van der Waals radii, the same against the WALL - the rows of ``drop_mask``, the pocket, when ``use_wall`` - and a
    harmonic restraint to the input position.  The topology is frozen at ``found``.  Heavy atoms only; no torsion,
    planarity or electrostatic term; at most 256 atoms after the pocket is dropped.  ``constants`` override
    ``const.RELAX_DEFAULTS``.

    ``mark_mask`` and ``drop_mask`` are ``[B,N]`` or ``[B,N,1]`` by row, ``atom_planar`` is ``[B,N]`` by atom number,
    ``bond_aromatic`` ``[B,capacity]`` by list entry.  Returns a ``Relaxed`` of device tensors: ``x [B,N,3]`` fp32, ``energy
    [B,2,5]`` fp64 (bonds, angles, repulsion, wall, restraint; before and after), ``steps_done [B]``, ``f_max [B]`` and
    ``moved2 [B]`` fp64 (the last largest |F| of an atom; the largest squared displacement) and ``status [B]``: the bits
    of ``found.status`` plus ``_lib.DL_POSE_*`` (more than 256 kept atoms or a non-finite coordinate: ``x`` comes back) and
    ``_lib.DL_RELAX_DIVERGED``."""
    unknown = sorted(set(constants) - set(const.RELAX_DEFAULTS))
    if unknown:
        raise TypeError(f'relax: unknown constants {unknown}; known: {sorted(const.RELAX_DEFAULTS)}')
    steps = int(steps)
    if not 0 <= steps <= _lib.DL_RELAX_MAX_STEPS:
        raise ValueError(f'steps must be 0..{_lib.DL_RELAX_MAX_STEPS}, got {steps}')
    others = tuple(m for m in (node_mask, drop_mask, mark_mask, atom_planar) if m is not None)
    _lib.require_device('relax', one_hot=one_hot, x=x, node_mask=node_mask, drop_mask=drop_mask, mark_mask=mark_mask,
                        atom_planar=atom_planar, bond_aromatic=bond_aromatic)
    B, N, nf = one_hot.shape
    if x.shape != (B, N, 3) or any(m.numel() != B * N for m in others):
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, x {tuple(x.shape)}, masks '
                         f'{[tuple(m.shape) for m in others]}')
    dev = one_hot.device
    given = normalize_bonds(found, B, dev, 'relax')
    capacity = given.bonds.shape[1]
    if bond_aromatic is not None and tuple(bond_aromatic.shape) != (B, capacity):
        raise ValueError(f'shapes disagree: bond_aromatic {tuple(bond_aromatic.shape)}, bonds {tuple(given.bonds.shape)}')
    one_hot, x, node_mask, drop_mask, mark_mask = (_lib.dense(t, dev, torch.float32)
                                                   for t in (one_hot, x, node_mask, drop_mask, mark_mask))
    if atom_planar is not None:
        atom_planar = _lib.dense(atom_planar.reshape(B, N) != 0, dev, torch.int32)
    if bond_aromatic is not None:
        bond_aromatic = _lib.dense(bond_aromatic != 0, dev, torch.int32)
    length0, aromatic0, ideal, reach = _relax_tables(dev, is_geom, reach_scale)
    if reach.shape[0] < nf:
        raise ValueError(f'one_hot has {nf} types, the vocabulary {reach.shape[0]}')
    if reach.shape[0] > nf:                                  # the kernel indexes the tables with nf
        length0, aromatic0, reach = (t[:nf, :nf].contiguous() for t in (length0, aromatic0, reach))
    values = dict(const.RELAX_DEFAULTS, **constants)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    out = Relaxed(torch.empty((B, N, 3), dtype=torch.float32, device=dev), f64(B, 2, _lib.DL_RELAX_TERMS), _lib.empty_i32(dev, B),
                  f64(B), f64(B), _lib.empty_i32(dev, B))
    args = _lib.DLRelaxArgs(
        B=B, N=N, nf=nf, x=x.data_ptr(), one_hot=one_hot.data_ptr(), node_mask=node_mask.data_ptr(), drop_mask=_lib.ptr(drop_mask),
        mark_mask=_lib.ptr(mark_mask), atom_planar=_lib.ptr(atom_planar), length0=length0.data_ptr(),
        aromatic_length0=aromatic0.data_ptr(), ideal_cos=ideal.data_ptr(), reach2=reach.data_ptr(), wall_reach2=reach.data_ptr(),
        capacity=capacity, n_bonds_in=given.n_bonds.data_ptr(), bonds=given.bonds.data_ptr() if capacity else None,
        bond_aromatic=_lib.ptr(bond_aromatic) if capacity else None, status_in=_lib.ptr(given.status),
        use_wall=int(bool(use_wall)), steps=steps, n_min=int(values['n_min']),
        x_out=out.x.data_ptr(), energy=out.energy.data_ptr(), steps_done=out.steps_done.data_ptr(), f_max=out.f_max.data_ptr(),
        moved2=out.moved2.data_ptr(), status=out.status.data_ptr(), **{name: float(values[name]) for name in _lib.RELAX_CONSTANTS})
    _lib.launch('dl_relax_molecules', args, dev)
    return out


def relax_samples(one_hot, x, node_mask, is_geom, linker_mask, drop_mask=None, margins=const.MARGINS_EDM, use_wall=True,
                  steps=const.RELAX_STEPS, **constants):
    """``relax`` of the linker atoms of every molecule of a batch, three launches and no host round trip between them:
    ``perceive_bonds``, ``refine_bond_orders`` and ``dl_relax_molecules``.  ALWAYS on the geometric (Kekule) orders, on
    ``atom_aromatic`` and on ``bond_aromatic``, whatever orders the files are written with, as ``metrics.analyze_pose_checks``
    does; the topology is that of the raw sample and stays frozen.  ``linker_mask`` and ``drop_mask`` (the pocket, which is
    also the wall) are ``[B,N]`` or ``[B,N,1]``.  Returns the ``Relaxed`` of ``relax``, which states the rule."""
    _lib.require_device('relax_samples', one_hot=one_hot, x=x, node_mask=node_mask, linker_mask=linker_mask)
    B, N = one_hot.shape[:2]
    if linker_mask.numel() != B * N:
        raise ValueError(f'shapes disagree: one_hot {tuple(one_hot.shape)}, linker_mask {tuple(linker_mask.shape)}')
    found = perceive_bonds(one_hot, x, node_mask, is_geom, margins)
    linker = linker_mask.reshape(B, N).to(torch.float32)
    refined, aromatic = refine_bond_orders(found, one_hot, x, node_mask, is_geom, drop_mask, linker)
    return relax(refined._replace(status=aromatic.status), one_hot, x, node_mask, is_geom, linker, drop_mask,
                 aromatic.atom_aromatic, aromatic.bond_aromatic, use_wall, steps, **constants)


def build_xae_molecules(one_hot, x, node_mask, is_geom, margins=const.MARGINS_EDM):
    """Per molecule the reference's ``(X, A, E)`` of ``build_xae_molecule``: atom types ``[n]`` (int64), adjacency
    ``[n,n]`` (bool) and bond orders ``[n,n]`` (int32), lower triangle only (the reference's graph is directed), dense, on
    the host."""
    found = perceive_all_bonds(one_hot, x, node_mask, is_geom, margins)
    n_bonds, bonds = found.n_bonds.cpu(), found.bonds.cpu().long()
    mask = node_mask.reshape(one_hot.shape[0], -1).cpu() != 0
    types = one_hot.detach().cpu().argmax(dim=2)
    out = []
    for b in range(one_hot.shape[0]):
        X = types[b][mask[b]]
        n = X.shape[0]
        E = torch.zeros((n, n), dtype=torch.int)
        rows = bonds[b, :int(n_bonds[b])]
        E[rows[:, 0], rows[:, 1]] = rows[:, 2].int()
        out.append((X, E.bool(), E))
    return out


def is_connected(one_hot, x, node_mask, is_geom, margins=const.MARGINS_EDM):
    """Device bool ``[B]``: the bond graph over the real atoms is one piece (``metrics.is_connected``:
    ``len(GetMolFrags(mol)) == 1`` of the molecule ``build_molecule`` makes from the same bonds)."""
    return perceive_bonds(one_hot, x, node_mask, is_geom, margins, capacity=0).n_components == 1


def summary(found):
    """The numbers the drivers print for a list of ``perceive_bonds`` results: molecules, the share in one piece and the
    mean bond count."""
    n_bonds = torch.cat([f.n_bonds for f in found]).float()
    one_piece = torch.cat([f.n_components for f in found]) == 1
    n = int(n_bonds.numel())
    return {'molecules': n, 'connected': float(one_piece.float().mean()) if n else 0.0,
            'mean_bonds': float(n_bonds.mean()) if n else 0.0}


_BOND_SYMBOL = {1: '', 2: '=', 3: '#'}


def _parity(keys):
    """+1 when sorting ``keys`` takes an even permutation, -1 when an odd one."""
    return -1 if sum(1 for q in range(len(keys)) for p in range(q) if keys[p] > keys[q]) % 2 else 1


def _direction_symbols(adj, when, classes, labelled):
    """The ``/`` and ``\\`` of a string: ``{(first written, second written): +1 for '/', -1 for '\\'}`` for the single bonds
    to the reference neighbours of the double bonds ``labelled`` (``{(a, b): 1 cis or 2 trans}``).  Read from a double-bond atom
    outward (the symbol as written when that atom is written first, reversed otherwise), equal symbols on the two ends of a
    double bond mean cis, and two symbols at one end differ.  A single bond that serves two double bonds (a diene) carries
    one symbol, so the symbols are the solution of a system of parities: every connected part of it starts with ``/`` on its
    bond written first.  A part whose parities contradict each other (possible in a conjugated ring only), and any part
    that would make the string state a configuration for a double bond that has none, is left without symbols."""
    def node(u, w):
        return (u, w) if when[u] < when[w] else (w, u)

    def outward(u, w):                               # the factor between the symbol of node(u, w) and its reading from u
        return 1 if when[u] < when[w] else -1

    reference, rules = {}, []
    for (a, b), label in labelled.items():
        ends = []
        for u, v in ((a, b), (b, a)):
            others = [w for w in adj[u] if w != v]
            if not 1 <= len(others) <= 2 or any(adj[u][w] != 1 for w in others):
                break
            ends.append(max(others, key=lambda w: classes[w]))
        else:
            reference[(a, b)] = ends
            rules.append((node(a, ends[0]), node(b, ends[1]), (1 if label == 1 else -1) * outward(a, ends[0]) * outward(b, ends[1])))
    nodes = sorted({n for rule in rules for n in rule[:2]}, key=lambda n: (when[n[0]], when[n[1]]))
    doubled = [u for u in range(len(adj)) if 2 in adj[u].values()]
    for u in doubled:                                # two arms at one end of a double bond are on opposite sides
        arms = [w for w in adj[u] if adj[u][w] == 1 and node(u, w) in nodes]
        if len(arms) == 2:
            rules.append((node(u, arms[0]), node(u, arms[1]), -outward(u, arms[0]) * outward(u, arms[1])))
    near = {n: [] for n in nodes}
    for n1, n2, product in rules:
        near[n1].append((n2, product))
        near[n2].append((n1, product))
    value, part_of, parts = {}, {}, []
    for start in nodes:
        if start in value:
            continue
        value[start], members, todo, sound = 1, [start], [start], True
        while todo:
            n1 = todo.pop()
            for n2, product in near[n1]:
                if n2 not in value:
                    value[n2] = value[n1] * product
                    members.append(n2)
                    todo.append(n2)
                elif value[n2] != value[n1] * product:
                    sound = False
        for n in members:
            part_of[n] = len(parts)
        parts.append(members if sound else [])
        if not sound:
            for n in members:
                del value[n]
    def arms(u, v):                                  # the single bonds at end u of the double bond (u, v) that carry a symbol
        return [node(u, w) for w in adj[u] if w != v and adj[u][w] == 1 and node(u, w) in value]

    pairs = [(u, v) for u in doubled for v in adj[u] if adj[u][v] == 2 and u < v]
    while True:                                      # no configuration for a double bond that has none
        stray = []
        for u, v in pairs:
            ends = reference.get((u, v)) and (u, v) or reference.get((v, u)) and (v, u)
            whole = ends and all(node(t, r) in value for t, r in zip(ends, reference[ends]))
            if arms(u, v) and arms(v, u) and not whole:
                stray = arms(u, v) + arms(v, u)
                break
        if not stray:
            return value
        for bond in stray:
            for n in parts[part_of[bond]]:
                value.pop(n, None)


def smiles(types, bonds, rank, classes=None, atom_stereo=None, bond_stereo=None):
    """One SMILES string for one molecule, on the host: ``types`` per atom (element indices of the vocabulary, or element
    symbols), ``bonds`` rows ``(i, j, order)`` with orders 1..3, ``rank`` a permutation of ``0..n-1`` per atom - the
    canonical ranks of ``metrics.canonical_ranks``, which make the string canonical under THIS project's rule.  It is NOT
    RDKit's canonical SMILES.

    Pieces are joined by ``.`` in the order of their smallest rank, and each starts at its atom of smallest rank.  The walk
    is depth first, neighbours in ascending rank; every child subtree but the last goes in parentheses, the bond symbol
    (none, ``=``, ``#``) in front of the child.  A bond to an atom already visited that is not the parent is a ring
    closure: at an atom its closures are listed in ascending rank of the partner; the end written first opens with the
    lowest free number (1..9, then ``%10``..``%99``) behind the bond symbol, the other end closes with the bare number.  A
    number is free again from the atom AFTER the one that closed it on, so no atom closes and opens the same number.  More
    than 99 numbers open at once: ``None``.  An atom is written bare when the sum of its bond orders is at most
    ``const.DEFAULT_VALENCE`` of its element and as ``[El]`` otherwise, so a reader's implicit hydrogens are those
    ``add_hydrogens`` places: none on an over-valent atom.  Orders are written as the list has them (Kekule forms, no
    aromatic lower case); no charges.  Nothing recurses: a chain of any length is walked with explicit stacks.

    STEREO.  With ``classes``, ``atom_stereo`` and ``bond_stereo`` all ``None`` there is none and the string is what it always
    was.  With them - ``classes`` and ``atom_stereo`` per atom and ``bond_stereo`` per row of ``bonds``, as ``metrics.stereo``
    perceives them - the string is an isomeric SMILES under THIS project's rule (NOT RDKit's, NOT CIP):

    - A centre (label 1 or 2) is written ``[C@H]``, ``[C@@H]``, ``[C@]`` or ``[C@@]``: the element, ``@`` or ``@@``, and ``H``
      when it has three neighbours.  Its neighbours in STRING ORDER are the preceding atom, then the implicit H, then the
      ring-closure digits in written order, then the children in written order.  ``@`` means: seen from the first of these,
      the others run anticlockwise - a NEGATIVE determinant ``det[n1 - n0, n2 - n0, n3 - n0]`` in that order in a right-handed
      frame - and ``@@`` clockwise.  Label 1 is a positive determinant in CLASS order (ascending ``classes``, the H lowest),
      so the symbol follows from the label and the parity of the permutation between the two orders.
    - A stereo double bond (label 1 cis, 2 trans, with respect to the neighbour of highest class at each end) puts ``/`` or
      ``\\`` on the single bonds to those two neighbours.  A symbol is read from the atom written first to the atom written
      second.  Re-expressed as read from the double-bond atom outward (reversing ``/`` and ``\\`` when the neighbour was written
      first), EQUAL symbols on the two ends mean cis: ``F/C=C\\F`` is cis, ``F/C=C/F`` trans.  A single bond that is the arm of two
      double bonds (a diene) carries one symbol that both agree with; a ring-closure bond carries its symbol at the opening
      digit and the complementary one at the closing digit (``_direction_symbols`` states the rare cases that get none).
    - Label 3 (undetermined) writes nothing."""
    n = len(types)
    symbol = [t if isinstance(t, str) else const.GEOM_IDX2ATOM[int(t)] for t in types]
    adj = [dict() for _ in range(n)]
    for i, j, order in bonds:
        adj[i][j] = order
        adj[j][i] = order
    near = [sorted(adj[u], key=lambda w: rank[w]) for u in range(n)]
    atom = [s if sum(adj[u].values()) <= const.DEFAULT_VALENCE[s] else f'[{s}]' for u, s in enumerate(symbol)]
    # first pass: the spanning forest of the walk, the order in which atoms are written, and the closures
    when, parent, children, closures, roots = [-1] * n, [-1] * n, [[] for _ in range(n)], [[] for _ in range(n)], []
    for root in sorted(range(n), key=lambda u: rank[u]):
        if when[root] >= 0:
            continue
        roots.append(root)
        when[root] = sum(1 for w in when if w >= 0)
        clock = when[root]
        stack = [(root, 0)]
        while stack:
            u, at = stack.pop()
            if at == len(near[u]):
                continue
            stack.append((u, at + 1))
            w = near[u][at]
            if when[w] < 0:
                clock += 1
                when[w], parent[w] = clock, u
                children[u].append(w)
                stack.append((w, 0))
            elif w != parent[u] and parent[w] != u and u not in closures[w]:
                closures[u].append(w)
                closures[w].append(u)
    slash = {}
    if classes is not None and atom_stereo is not None and bond_stereo is not None:
        for u in range(n):
            if atom_stereo[u] in (1, 2) and len(adj[u]) in (3, 4) and all(o == 1 for o in adj[u].values()):
                around = ([parent[u]] if parent[u] >= 0 else []) + ([-1] if len(adj[u]) == 3 else []) \
                    + sorted(closures[u], key=lambda v: rank[v]) + children[u]
                sign = (1 if atom_stereo[u] == 1 else -1) * _parity([-1 if w < 0 else classes[w] for w in around])
                atom[u] = f'[{symbol[u]}{"@@" if sign > 0 else "@"}{"H" if len(adj[u]) == 3 else ""}]'
        labelled = {(i, j): label for (i, j, order), label in zip(bonds, bond_stereo) if label in (1, 2) and adj[i][j] == 2}
        slash = {pair: '/' if v > 0 else '\\' for pair, v in _direction_symbols(adj, when, classes, labelled).items()}
    turned = {'/': '\\', '\\': '/', '': ''}
    # second pass: the text
    free, number, parts = list(range(1, 100)), {}, []
    for root in roots:
        out, todo = [], [('atom', root, '')]
        while todo:
            kind, u, bond = todo.pop()
            if kind == 'text':
                out.append(bond)
                continue
            out.append(bond + atom[u])
            closed = []
            for w in sorted(closures[u], key=lambda v: rank[v]):
                pair = (min(u, w), max(u, w))
                if pair in number:
                    k = number.pop(pair)
                    closed.append(k)
                    out.append(turned[slash.get((w, u), '')] + (str(k) if k < 10 else f'%{k}'))
                else:
                    if not free:
                        return None
                    k = free.pop(0)
                    number[pair] = k
                    out.append(_BOND_SYMBOL[adj[u][w]] + slash.get((u, w), '') + (str(k) if k < 10 else f'%{k}'))
            free = sorted(free + closed)
            kids = children[u]
            for at in range(len(kids) - 1, -1, -1):
                w = kids[at]
                if at < len(kids) - 1:
                    todo.append(('text', -1, ')'))
                    todo.append(('atom', w, _BOND_SYMBOL[adj[u][w]] + slash.get((u, w), '')))
                    todo.append(('text', -1, '('))
                else:
                    todo.append(('atom', w, _BOND_SYMBOL[adj[u][w]] + slash.get((u, w), '')))
        parts.append(''.join(out))
    return '.'.join(parts)
