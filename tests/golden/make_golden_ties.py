"""Generate ``cutoff_ties.npz`` from the UNMODIFIED reference: what it decides for pairs that lie EXACTLY on a distance
cut-off, on the lattice molecules of tests/lattice_cases.py.

Run in the build container only (it imports the reference, which does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ties.py

RDKit and the other packages the reference imports at module top are replaced by the stand-ins of
``make_golden._stub_reference_dependencies``; no function used here touches them.  The file holds data only (inputs and
recorded outputs) and is written with fixed zip time stamps, so a second run reproduces it bit for bit.

``bonds.<zinc|geom>.*``    ``one_hot [B,64,nf]``, ``x``, ``mask`` of ``lattice_bond_molecules`` and ``E [B,60,60]``: the matrix of
                           ``build_xae_molecule`` (src/molecule_builder.py:44-75) for the real atoms of every molecule, zero-padded.
``pocket.<graph>.*``       the inputs of ``lattice_pocket_case(graph)``, ``out``: ``DynamicsWithPockets.forward`` (src/egnn.py:471-552)
                           with the weights ``seeded_state_dict(12, 128, 2, 31)`` - the recipe of ``make_golden.pocket_forward`` - and
                           ``edges``: ``get_dist_edges`` / ``get_dist_edges_4A`` (:554-596) on the same coordinates.
``size.*``                 the batch of ``lattice_size_case``, the logits of the reference ``SizeGNN`` driven as
                           ``SizeClassifier.forward`` drives it (the recipe of ``make_golden.size_gnn``; models 'plain' and 'bn'), from
                           the positions and (``logits_given_*``) from the case's given squared distances, and the kept edges.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden                                          # noqa: E402  (sets sys.path: repository, tests/, reference)
from make_golden_bonds import save_deterministic            # noqa: E402  (stubs the reference's optional dependencies)

from src.egnn import DynamicsWithPockets, coord2diff        # noqa: E402
from src.linker_size import SizeGNN                         # noqa: E402
from src.molecule_builder import build_xae_molecule         # noqa: E402

import lattice_cases as LC                                  # noqa: E402

MAX_ATOMS = 60


def bonds():
    out = {}
    for is_geom, tag in ((False, 'zinc'), (True, 'geom')):
        case = LC.lattice_bond_molecules(is_geom)
        assert LC.problems(case, with_reference=False) == []
        E_all = np.zeros((len(case.mols), MAX_ATOMS, MAX_ATOMS), np.int8)
        for b, (name, kinds, pos) in enumerate(case.mols):
            _, A, E = build_xae_molecule(torch.from_numpy(pos), torch.from_numpy(kinds), is_geom=is_geom)
            assert torch.equal(A, E.bool())
            E_all[b, :len(kinds), :len(kinds)] = E.numpy()
        out.update({f'bonds.{tag}.one_hot': case.one_hot, f'bonds.{tag}.x': case.x, f'bonds.{tag}.mask': case.mask,
                    f'bonds.{tag}.E': E_all})
    return out


@torch.no_grad()
def pockets():
    out = {}
    for graph in LC.GRAPHS:
        case = LC.lattice_pocket_case(graph)
        inp, z, t = case.inp, case.z, case.t
        B, N = z.shape[:2]
        dyn = make_golden.ref_dynamics(DynamicsWithPockets, LC.NF, 2, LC.POCKET_WEIGHTS['n_layers'], graph,
                                       seed=LC.POCKET_WEIGHTS['seed'])
        res = dyn.forward(t=t, xh=z, node_mask=inp['node_mask'], linker_mask=inp['linker_mask'], edge_mask=inp['edge_mask'],
                          context=inp['context'])
        assert torch.isfinite(res).all()
        nm = inp['node_mask'].view(B * N, 1)
        x = (z.view(B * N, -1) * nm)[:, :3]
        if graph == '4A':
            edges = dyn.get_dist_edges_4A(x, nm, inp['edge_mask'])
        else:
            edges = dyn.get_dist_edges(x, nm, inp['edge_mask'], inp['linker_mask'].view(B * N, 1),
                                       inp['context'][..., -2].reshape(B * N, 1), inp['context'][..., -1].reshape(B * N, 1))
        pre = f'pocket.{graph}.'
        out.update({pre + 'xh': z, pre + 't': t, pre + 'out': res, pre + 'edges': edges.to(torch.int32), pre + 'seed': case.seed})
        out.update({pre + k: inp[k] for k in ('x', 'h', 'node_mask', 'fragment_mask', 'linker_mask', 'edge_mask', 'context')})
    return out


@torch.no_grad()
def size():
    case = LC.lattice_size_case()
    assert LC.problems(case, with_reference=False) == []
    data = case.data
    out = {'size.' + k: data[k] for k in ('one_hot', 'positions', 'fragment_mask', 'linker_mask', 'edge_mask')}
    out['size.distances'] = case.distances
    for tag, (n_layers, bn) in LC.SIZE_MODELS.items():
        gnn = SizeGNN(in_node_nf=LC.SIZE_IN_NF, hidden_nf=128, out_node_nf=LC.SIZE_OUT_NF, n_layers=n_layers,
                      normalization='batch_norm' if bn else None)
        gnn.load_state_dict({k[4:]: v for k, v in LC.size_state_dict(tag).items()}, strict=True)
        gnn.eval()
        h, x = data['one_hot'], data['positions']
        fragment_mask, edge_mask, edges = data['fragment_mask'], data['edge_mask'], data['edges']
        x = x * fragment_mask                                  # linker_size_lightning.py:83-110
        h = h * fragment_mask
        bs, n_nodes = x.shape[0], x.shape[1]
        fm = fragment_mask.view(bs * n_nodes, 1)
        for name, distances in (('', coord2diff(x.view(bs * n_nodes, -1), edges)[0]), ('_given', case.distances.reshape(-1, 1))):
            distance_edge_mask = (edge_mask.bool() & (distances < 6)).long()
            output = gnn.forward(h.view(bs * n_nodes, -1), edges, distances, fm, distance_edge_mask)
            out[f'size.logits{name}_{tag}'] = output.view(bs, n_nodes, -1).mean(1)
            out[f'size.kept{name}'] = distance_edge_mask.view(bs, n_nodes, n_nodes).to(torch.int8)
    return out


if __name__ == '__main__':
    torch.set_num_threads(1)
    arrays = {**bonds(), **pockets(), **size()}
    save_deterministic('cutoff_ties', {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()})
