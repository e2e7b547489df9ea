"""Frame and numbering independence of the 3D analysis kernels: every entry point of ``tests/frame_cases.py`` run once on a base
case and once on the same molecules rotated, mirrored, moved 100 to 300 A away or renumbered, in one process and on fresh
tensors, and compared after ``undo`` - discrete outputs exactly, continuous ones within the bars stated there.  Nothing here
compares with a restatement's result: a kernel is held to ITSELF, so what a kernel and its restatement share is seen too.
(One INPUT comes from a restatement: the ``xs_type`` handed to ``dl_interaction_scores`` in case 'own_targets' is
``interaction_ref.interaction_types`` of the same frame; ``dl_interaction_types`` itself is an entry point of its own here.)

Every entry point is reached through the ``launch`` / ``score`` helper of its own GPU test module (``dl_perceive_bonds``
through ``perceive_bonds``, which is that module's way in), and the three-launch chains through their wrappers:
``perceive_bonds`` -> ``refine_bond_orders`` -> ``add_hydrogens``, ``analyze_pose_checks`` and ``relax_samples``;
``analyze_clashes`` is ``test_gpu_clash.score`` itself and ``analyze_interactions`` carries the shared protein list of 257."""
import numpy as np
import pytest
import torch

import frame_cases as fc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BASE = {}
WORST = {}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def host(result, names=None):
    """A dict of numpy arrays of a dict or namedtuple of tensors."""
    items = result.items() if isinstance(result, dict) else zip(result._fields, result)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in items if names is None or k in names}


# ---- the kernels, by entry point ---------------------------------------------------------------------------------------------------
def bonds(e, inputs, run):
    from difflinker_amd.molecule_builder import perceive_bonds
    from test_gpu_bonds import every_pair
    found = host(perceive_bonds(dev(inputs['one_hot']), dev(inputs['x']), dev(inputs['mask']), False,
                                capacity=every_pair(inputs['mask'].shape[1])))
    found['bonds'] = [found['bonds'][b, :n].tolist() for b, n in enumerate(found['n_bonds'])]
    return found


def aromatic(e, inputs, run):
    import test_gpu_aromatic as AR
    return AR.launch(inputs)


def hydrogens(e, inputs, run):
    import test_gpu_hydrogens as TH
    return TH.launch(inputs)


def pose_checks(e, inputs, run):
    import test_gpu_pose_checks as TP
    return TP.launch(inputs)


def relax(e, inputs, run):
    import test_gpu_relax as TR
    return TR.launch(inputs, steps=run)


def clash(e, inputs, run):
    import test_gpu_clash as CL
    protein = (inputs['protein_x'], inputs['protein_type']) if 'protein_x' in inputs else None
    return host(CL.score(inputs['x'], inputs['one_hot'], inputs['qm'], inputs['tm'], protein=protein))


def interaction_types(e, inputs, run):
    import test_gpu_interaction as TI
    xs, status = TI.launch_types(inputs['x'], inputs['one_hot'], inputs['group'])
    return dict(xs_type=xs.cpu().numpy(), status=status.cpu().numpy())


def interaction_scores(e, inputs, run):
    import test_gpu_interaction as TI
    if 'protein_x' in inputs:                      # the shared list goes in through the wrapper, which types with the kernel
        return host(TI.analyze(inputs['x'], inputs['one_hot'], inputs['qm'], inputs['lig'], inputs['tm'],
                               protein=(inputs['protein_x'], inputs['protein_xs'])))
    return host(TI.launch_scores(inputs['x'], inputs['xs_type'], inputs['qm'], inputs['tm']))


def pharmacophore(e, inputs, run):
    import test_gpu_pharmacophore as TP
    return host(TP.launch(inputs, e.FCAP, None, inputs['mark']))


def feature_match(e, inputs, run):
    import test_gpu_pharmacophore as TP
    return host(TP.launch_match(inputs['a'], inputs['b'], e.RADIUS2))


def shape(e, inputs, run):
    import test_gpu_shape as SH
    return SH.as_dict(SH.score(e.arrays(inputs)))


def rmsd(e, inputs, run):
    import test_gpu_rmsd as RM
    cases = [(str(p), pair['a'], pair['b'], pair['maps'], None) for p, pair in enumerate(inputs['pairs'])]
    value, best, status = RM.launch(cases, max(len(pair['a']) for pair in inputs['pairs']) + 1)
    return dict(rmsd=value.numpy().astype(np.float64), best=best.numpy(), status=status.numpy())


def pocket(e, inputs, run):
    import test_gpu_pocket as PK
    return PK.launch(inputs, e.R)


def chain_bonds(inputs, found):
    """What the wrappers derived, written into ``inputs`` for ``compare`` (as ``frame_cases.Chain.reference`` does)."""
    B = len(inputs['mask'])
    n_in, rows = found.n_bonds.cpu().numpy(), found.bonds.cpu().numpy()
    inputs.update(bonds=rows, n_in=n_in, n_bonds_in=n_in)
    return [sorted((min(i, j), max(i, j)) for i, j, _ in rows[b, :n_in[b]].tolist()) for b in range(B)]


def chain_tensors(inputs):
    return dev(inputs['one_hot']), dev(inputs['x']), dev(inputs['mask'])


def chain_hydrogens(e, inputs, run):
    from difflinker_amd.molecule_builder import add_hydrogens, perceive_bonds, refine_bond_orders
    one_hot, x, mask = chain_tensors(inputs)
    found = perceive_bonds(one_hot, x, mask, False)
    refined, arom = refine_bond_orders(found, one_hot, x, mask, False, dev(inputs['drop']), dev(inputs['mark']))
    got = add_hydrogens(refined._replace(status=arom.status), one_hot, x, mask, False, dev(inputs['drop']), arom.atom_aromatic)
    out = dict(n_h=got.n_h, h_count=got.h_count, h_parent=got.parent, h_x=got.x, status=got.status, n_aromatic_rings=arom.n_aromatic_rings)
    out = host(out)
    out['chain_bonds'] = chain_bonds(inputs, refined)
    inputs.update(planar=arom.atom_aromatic.cpu().numpy())
    return out


def chain_pose_checks(e, inputs, run):
    from difflinker_amd.metrics import analyze_pose_checks
    one_hot, x, mask = chain_tensors(inputs)
    got = analyze_pose_checks(one_hot, x, mask, False, dev(inputs['mark']), dev(inputs['drop']))
    out = host(dict(counts=got.counts, atom_flags=got.atom_flags, status=got.status, n_aromatic_rings=got.aromatic.n_aromatic_rings))
    out['chain_bonds'] = chain_bonds(inputs, got.refined)
    return out


def chain_relax(e, inputs, run):
    from difflinker_amd.molecule_builder import perceive_bonds, refine_bond_orders, relax_samples
    one_hot, x, mask = chain_tensors(inputs)
    got = relax_samples(one_hot, x, mask, False, dev(inputs['mark']), dev(inputs['drop']), steps=run)
    found = perceive_bonds(one_hot, x, mask, False)                       # the list the wrapper derived, once more, for the comparison
    refined, arom = refine_bond_orders(found, one_hot, x, mask, False, dev(inputs['drop']), dev(inputs['mark']))
    out = host(dict(x_out=got.x, energy=got.energy, steps_done=got.steps_done, f_max=got.f_max, moved2=got.moved2, status=got.status,
                    n_aromatic_rings=arom.n_aromatic_rings))
    out['chain_bonds'] = chain_bonds(inputs, refined)
    return out


KERNELS = {'dl_perceive_bonds': bonds, 'dl_aromatic_rings': aromatic, 'dl_add_hydrogens': hydrogens, 'dl_pose_checks': pose_checks,
           'dl_clash_scores': clash, 'dl_interaction_types': interaction_types, 'dl_interaction_scores': interaction_scores,
           'dl_pharmacophore_features': pharmacophore, 'dl_feature_match': feature_match, 'dl_shape_scores': shape,
           'dl_best_rmsd': rmsd, 'dl_relax_molecules': relax, 'dl_pocket_select': pocket,
           'chain:add_hydrogens': chain_hydrogens, 'chain:analyze_pose_checks': chain_pose_checks, 'chain:relax_samples': chain_relax}


def kernel(e, inputs, run):
    return KERNELS[e.name](e, inputs, run)


def note(entry, transform, run, measured):
    """The largest deviation seen per entry point and kind of transform, printed with every test that raises it."""
    if measured is None:
        return
    values = measured if isinstance(measured, dict) else {'': measured}
    for name, value in values.items():
        key = (entry, fc.TRANSFORMS[transform].kind, run, name)
        if value > WORST.get(key, -1):
            WORST[key] = value
            print(f'{entry} {name} steps={run} {transform}: largest deviation so far {value:.3e}')


def test_every_entry_point_has_its_kernel():
    assert set(KERNELS) == set(fc.ENTRY_POINTS) and len(fc.ENTRIES) == 13


@pytest.mark.parametrize('entry,case_name,transform,run', fc.parameters())
def test_kernel_is_frame_and_numbering_free(entry, case_name, transform, run):
    note(entry, transform, run, fc.check(kernel, entry, case_name, transform, run, BASE))


@pytest.mark.parametrize('entry,case_name,transform,run', fc.parameters(fc.CHAINS))
def test_wrapper_chain_is_frame_and_numbering_free(entry, case_name, transform, run):
    """The chain as a whole, the intermediate bond list included."""
    note(entry, transform, run, fc.check(kernel, entry, case_name, transform, run, BASE))


def test_relax_f_is_a_length():
    """The regression case of what this suite found in the rule of ``dl_relax_molecules``: ``f`` was the largest force
    COMPONENT, which a rotation changes by up to sqrt(3), and with it ``f_max`` and the step at which a run meets ``f_tol``.
    It is the largest |F| of an atom now, in the header, the restatement and the kernel together.  One movable atom pulled
    by one bond with |F| = 20, along the diagonal and along x: the two agree at every ``f_tol``, where an ``f_tol`` between
    |F| / sqrt(3) and |F| used to end the diagonal one alone."""
    import relax_ref as rr
    import test_gpu_relax as TR
    far = 1.54 + 0.1
    diagonal = fc.molecule_of([0, 0], [(0, 0, 0), (far / np.sqrt(3),) * 3], [(1, 0, 1)], marked=[1])
    along_x = fc.molecule_of([0, 0], [(0, 0, 0), (far, 0, 0)], [(1, 0, 1)], marked=[1])
    batch = fc.pack([fc.moved(m, fc.IDENTITY, b) for b, m in enumerate((diagonal, along_x))], 4, 1)
    force = 2 * rr.DEFAULTS['k_bond'] * 0.1
    for f_tol, steps in ((0.5 * force, [1, 1]), (0.8 * force, [1, 1]), (1.2 * force, [0, 0])):
        got = TR.launch(batch, steps=1, f_tol=f_tol)
        assert got['steps_done'].tolist() == steps and np.allclose(got['f_max'], force, rtol=1e-4), (f_tol, got['steps_done'], got['f_max'])
