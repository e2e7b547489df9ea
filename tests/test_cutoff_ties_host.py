"""The lattice cases of tests/lattice_cases.py on the CPU: their preconditions, the oracles against what the unmodified
reference recorded for them (tests/golden/cutoff_ties.npz), and DISCRIMINATION - the same fp64 oracle with one comparison
flipped (``<`` for ``<=`` in the radius graphs, ``<=`` for ``<`` in the bond rule and in the size predictor's filter) must
differ from the true one by at least 20 times the loosest bar tests/test_gpu_cutoff_ties.py applies, so none of its tests can
pass with the wrong operator.

Measured (fp64 oracle, flipped against true; bar = the loosest one of the GPU test; ratio = measured / bar):

    pocket forward, h, bar 1e-5 (FWD_TOLS['fp32'])     FC-10A-4A 5.6e-3 (564)   FC-4A 1.5e-3 (147)   4A 1.6e-3 (156)
        one comparison of the FC graphs flipped alone: pocket-pocket 1.1e-3 (111) / 1.2e-3 (122), ligand-pocket 5.5e-3 (553) /
        7.5e-4 (75, the worst ratio of this file)
    pocket forward, x + vel (coordinate head gain 0.02) 3.3e-5 / 5.8e-6 / 7.9e-6: no evidence either way, not asserted
    pocket backward, all parameters, bar 2e-6           FC-10A-4A 9.7e-3 (4800)  FC-4A 2.7e-3 (1300)
    pocket backward, worst tensor, bar 1e-5             FC-10A-4A 0.14 (13000)   FC-4A 0.11 (10000)
        one comparison alone: at least 9.9e-4 over all parameters (496) and 3.3e-2 on the worst tensor (3272)
        tensors that do not reach 20 bars: ``embedding_out.bias`` (its gradient is the column sum of the cotangent, whatever the
        graph: 0), ``e_block_1.gcl_1.node_mlp.2.bias`` (3e-6: the last node update feeds embedding_out alone) and, under FC-4A,
        ``e_block_1.gcl_0.node_mlp.2.bias`` (1.8e-4 against 2e-4); every other tensor is asserted
    size predictor, logits, bar 1e-5                    plain 6.6e-2 (6600)      bn 5.6e-2 (5600)
    bonds, entries of E that change                     ZINC 26, GEOM 28; the split molecule: 2 pieces -> 1
    pocket chain, T = 6, FC-10A-4A, bar 1e-4 (CHAIN_TOL): the flipped chain moves the final linker coordinates by 1.4e-7 (gain
        0.02), 5.3e-7 (0.1), 1.2e-6 (0.2) and the other frames by 1.4e-6; from gain 0.5 on the oracle chain is not finite.  Far
        below 20 bars at every usable gain, so a chain test could pass with the wrong operator: the GPU file has none
        (``test_a_chain_cannot_tell_the_operators_apart`` keeps the record).
"""
import numpy as np
import pytest
import torch

import lattice_cases as LC
import test_gpu_pocket_train as PT
from helpers import max_abs, rel_l2
from oracle import egnn_oracle, size_oracle
from test_gpu_parity import CHAIN_TOL, FWD_TOLS
from test_gpu_size_gnn import TOL as SIZE_TOL

FACTOR = 20
# gradient tensors the flipped graph moves by less than FACTOR * BAR_TENSOR (module docstring)
QUIET = {'FC-10A-4A': {'dynamics.embedding_out.bias', 'dynamics.e_block_1.gcl_1.node_mlp.2.bias'},
         'FC-4A': {'dynamics.embedding_out.bias', 'dynamics.e_block_1.gcl_1.node_mlp.2.bias',
                   'dynamics.e_block_1.gcl_0.node_mlp.2.bias'}}


def all_cases():
    return [LC.lattice_pocket_case(g) for g in LC.GRAPHS] + [LC.lattice_bond_molecules(False), LC.lattice_bond_molecules(True),
                                                            LC.lattice_size_case()]


def test_every_case_meets_its_preconditions():
    for case in all_cases():
        assert LC.problems(case) == []


def test_seed_search_ends_at_its_first_candidate():
    for graph in LC.GRAPHS:
        assert LC.lattice_pocket_case(graph).seed == LC.POCKET_SEEDS[graph]


def test_tie_counts():
    """Per molecule at least 6 pocket-pocket and 8 ligand-pocket ties, one coincident pair."""
    for graph in LC.GRAPHS:
        for info in LC.pocket_tie_counts(LC.lattice_pocket_case(graph)):
            c = info['counts']
            assert c['PP'] >= 6 and c['FP'] >= 4 and c['LP'] >= 4 and info['coincident'] >= 1, (graph, info)
    assert min(LC.size_tie_counts(LC.lattice_size_case())) >= 8


@pytest.mark.parametrize('graph', LC.GRAPHS)
def test_pocket_oracle_reproduces_the_reference(graph):
    case = LC.lattice_pocket_case(graph)
    fix = LC.fixture()
    B, N = case.z.shape[:2]
    inp = case.inp
    nm = inp['node_mask'].view(B * N, 1)
    x = (case.z.view(B * N, -1) * nm)[:, :3]
    masks = (inp['edge_mask'].view(-1), inp['linker_mask'].view(B * N, 1), inp['context'][..., -2].reshape(B * N, 1),
             inp['context'][..., -1].reshape(B * N, 1))
    want = torch.from_numpy(fix[f'pocket.{graph}.edges']).long()
    for dtype in (torch.float32, torch.float64):
        row, col = egnn_oracle.pocket_edges(LC.pocket_config(graph), x.to(dtype), nm.to(dtype), *masks)
        assert torch.equal(torch.stack([row, col]), want), dtype
    row, col = LC.flipped_pocket_edges(LC.pocket_config(graph), x.double(), nm.double(), *masks)
    ties = sum(sum(info['counts'].values()) for info in LC.pocket_tie_counts(case))
    assert want.shape[1] - len(row) == 2 * ties, 'the flipped graph loses exactly the ties, in both directions'
    out = LC.pocket_oracle_forward(case, dtype=torch.float32)
    ref = torch.from_numpy(fix[f'pocket.{graph}.out'])
    assert torch.isfinite(ref).all() and max_abs(out, ref) <= 1e-6               # the bar of tests/test_oracle_golden.py


@pytest.mark.parametrize('is_geom', [False, True])
def test_bond_restatement_reproduces_the_reference(is_geom):
    case = LC.lattice_bond_molecules(is_geom)
    E_ref = LC.fixture()[f'bonds.{"geom" if is_geom else "zinc"}.E']
    changed, orders = 0, set()
    for b, (name, kinds, pos) in enumerate(case.mols):
        n = len(kinds)
        E = LC.bond_matrix(is_geom, kinds, pos)
        assert np.array_equal(E, E_ref[b][:n, :n]), name
        assert not E_ref[b][n:].any() and not E_ref[b][:, n:].any()
        flipped = LC.bond_matrix(is_geom, kinds, pos, LC.bond_order_flipped)
        changed += int((flipped != E).sum())
        orders |= set(np.unique(E).tolist())
        if name.startswith('split'):
            assert LC.pieces(E) == 2 and LC.pieces(flipped) == 1, name
    assert changed >= 8 and orders == {0, 1, 2, 3}, (changed, orders)


@pytest.mark.parametrize('tag', list(LC.SIZE_MODELS))
def test_size_oracle_reproduces_the_reference_and_tells_the_operators_apart(tag):
    case = LC.lattice_size_case()
    fix = LC.fixture()
    d = case.data
    L, bn = LC.SIZE_MODELS[tag]
    out = size_oracle.size_classifier_logits(LC.size_state_dict(tag), d['one_hot'], d['positions'], d['fragment_mask'],
                                             d['edge_mask'], L, batch_norm=bn)
    assert torch.equal(out, LC.size_logits(case, tag, dtype=torch.float32)), 'the restatement with the filter as a parameter'
    for name, distances in (('', None), ('_given', case.distances)):
        ref = torch.from_numpy(fix[f'size.logits{name}_{tag}'])
        got = LC.size_logits(case, tag, dtype=torch.float32, distances=distances)
        assert max_abs(got, ref) <= 2e-6 and rel_l2(got, ref) <= 1e-6, name      # the bars of tests/test_oracle_golden.py
        true = LC.size_logits(case, tag, distances=distances)
        flipped = LC.size_logits(case, tag, distances=distances, keep=lambda r: r <= 6)
        moved = rel_l2(flipped, true)
        print(f'[size {tag}{name}] flipped filter moves the logits by {moved:.2e}: {moved / SIZE_TOL:.0f} bars')
        assert moved >= FACTOR * SIZE_TOL
    # the two neighbours of 6 in the given distances fall on their own sides in the reference's recorded mask
    kept = fix['size.kept_given']
    assert kept[0, 0, 1] == 1 and kept[0, 1, 2] == 0 and fix['size.kept'][0, 0, 1] == 0
    assert rel_l2(LC.size_logits(case, tag, distances=case.distances), LC.size_logits(case, tag)) >= FACTOR * SIZE_TOL


MUTANTS = [(g, w) for g in LC.GRAPHS for w in (('all',) if g == '4A' else ('all', 'pocket', 'cross'))]


@pytest.mark.parametrize('graph,which', MUTANTS)
def test_flipped_graph_moves_the_forward(graph, which):
    """``which``: every comparison of ``pk_adjacent`` flipped, or one of them alone."""
    case = LC.lattice_pocket_case(graph)
    true = LC.pocket_oracle_forward(case)
    with LC.flipped_graph(which):
        flipped = LC.pocket_oracle_forward(case)
    assert torch.isfinite(true).all() and torch.isfinite(flipped).all()          # the coincident pair included
    moved = rel_l2(flipped[..., 3:], true[..., 3:])
    bar = max(FWD_TOLS.values())
    print(f'[pocket forward {graph}, {which}] flipped graph moves h by {moved:.2e}: {moved / bar:.0f} bars')
    assert moved >= FACTOR * bar
    assert torch.equal(LC.pocket_oracle_forward(case), true), 'the true oracle is back in place'


@pytest.mark.parametrize('graph,which', [m for m in MUTANTS if m[0] != '4A'])
def test_flipped_graph_moves_the_gradient(graph, which):
    case = LC.lattice_pocket_case(graph)
    G = LC.cotangent(case)
    true = LC.pocket_oracle_grads(case, G)
    with LC.flipped_graph(which):
        flipped = LC.pocket_oracle_grads(case, G)
    total, worst = PT.compare(flipped, true)
    per = {k: rel_l2(flipped[k], true[k]) for k in true}
    print(f'[pocket backward {graph}, {which}] flipped graph: all {total:.2e} ({total / PT.BAR_ALL:.0f} bars), worst tensor '
          f'{worst:.2e} ({worst / PT.BAR_TENSOR:.0f} bars)')
    assert total >= FACTOR * PT.BAR_ALL and worst >= FACTOR * PT.BAR_TENSOR
    if which == 'all':
        assert {k for k, v in per.items() if v < FACTOR * PT.BAR_TENSOR} == QUIET[graph]


def test_a_chain_cannot_tell_the_operators_apart():
    """The record behind leaving the chain out of the GPU file: at every coordinate-head gain at which the oracle chain stays
    finite, flipping the comparison moves the compared quantities by far less than one ``CHAIN_TOL``."""
    case = LC.lattice_pocket_case('FC-10A-4A')
    lm = case.inp['linker_mask']
    for gain in (0.02, 0.2):
        want, _ = LC.pocket_oracle_chain(case, 6, 39, gain)
        with LC.flipped_graph():
            flipped, _ = LC.pocket_oracle_chain(case, 6, 39, gain)
        assert torch.isfinite(want).all()
        moved = max(rel_l2(flipped[0, :, :, :3] * lm, want[0, :, :, :3] * lm), rel_l2(flipped[1:], want[1:]))
        print(f'[pocket chain, gain {gain}] flipped graph moves the chain by {moved:.2e}')
        assert 0 < moved < CHAIN_TOL / FACTOR


@pytest.mark.parametrize('name', list(LC.FC_COINCIDENT))
def test_the_oracle_is_finite_where_atoms_coincide(name):
    inp, z, t = LC.fc_coincident_case(name)
    x = z[..., :3] * inp['node_mask']
    real = inp['node_mask'][..., 0] != 0
    same = (torch.cdist(x, x) == 0) & real[:, :, None] & real[:, None, :]
    assert int(same.sum()) - int(real.sum()) >= 2, 'two real atoms at one point'
    G = torch.randn(z.shape, generator=torch.Generator().manual_seed(3))
    for dtype in (torch.float32, torch.float64):
        out, grads = LC.fc_oracle(name, G, dtype)
        assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads.values()), dtype
