"""Every distance cut-off of the kernels AT the tie: the lattice molecules of tests/lattice_cases.py, whose pairs lie exactly
on a cut-off (or one fp32 step beside it) and whose squared distances are exact in fp32 under any formula, so that a kernel
and its reference can only disagree through the comparison operator.

    radius graphs  ``<= 4`` / ``<= 10`` (egnn.py:554-596)        pk_adjacent, csrc/egnn_sparse.hip; adjacent, csrc/egnn_backward_sparse.hip
    bond order     ``100 * d < T`` (molecule_builder.py:90-98)    pair_order, csrc/bonds.hip, and what reads its list
    size GNN       squared distance ``< 6`` (linker_size_lightning.py:107)   csrc/size_gnn.hip, csrc/size_gnn_train.hip

References: the fp64 oracle, and what the unmodified reference recorded on the same inputs (tests/golden/cutoff_ties.npz).
No bar is new: the ones of tests/test_gpu_parity.py, test_gpu_pocket_train.py, test_gpu_train.py, test_gpu_size_gnn.py and
test_gpu_size_train.py.  tests/test_cutoff_ties_host.py shows on the CPU that flipping any of the comparisons moves every
compared quantity by at least 20 of these bars (bonds: changes at least 8 entries of ``E`` and the piece count), so no test
here passes with the wrong operator.  No pair of any molecule is excluded from any comparison.

There is no chain test: a 6-step pocket chain with the flipped graph stays within 1.4e-6 of the true one, far inside
``CHAIN_TOL`` (tests/test_cutoff_ties_host.py::test_a_chain_cannot_tell_the_operators_apart), so it could not fail.
"""
import numpy as np
import pytest
import torch

import independence_cases as IC
import lattice_cases as LC
import test_gpu_parity as P
import test_gpu_pocket_train as PT
import test_gpu_size_gnn as SG
import test_gpu_size_train as ST
import test_gpu_train as FT
from helpers import rel_l2
from oracle import size_oracle

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
PRECISIONS = ('f16x3', 'fp32')


def errors(tag, out, ref, z):
    """rel-L2 on ``x + vel`` and on ``h`` against an fp64 reference.  ``P.report`` also bounds the RAW velocity by 1e-4; against
    fp64 that figure is the fp32 rounding of ``x_final`` itself (one ulp of a coordinate of 10 - 20 A is 1 - 2e-6 A, the whole
    update of a sparse graph with the 0.02-gain head is a few 1e-3 A), not an error of the update: measured 2.2e-4 on '4A' with
    ``x + vel`` at 6.5e-9 and the raw velocity against the fp32 reference fixture at 1e-8.  So the raw bar is applied where the
    reference is fp32, as everywhere else in the suite, and printed here."""
    x0 = z[..., :3].double()
    ev = rel_l2(x0 + out[..., :3].double(), x0 + ref[..., :3].double())
    eh = rel_l2(out[..., 3:], ref[..., 3:])
    print(f'[{tag}] rel-L2 x+vel {ev:.3e} (raw vel {rel_l2(out[..., :3], ref[..., :3]):.3e}) h {eh:.3e}')
    return ev, eh


# ---- radius graphs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('graph', LC.GRAPHS)
def test_pocket_forward_at_the_ties(graph, precision):
    case = LC.lattice_pocket_case(graph)
    inp, z, t = case.inp, case.z, case.t
    tol = P.FWD_TOLS[precision]
    dyn, _, _ = P.make_pocket_dynamics(LC.NF, LC.POCKET_WEIGHTS['n_layers'], seed=LC.POCKET_WEIGHTS['seed'], graph_type=graph,
                                       precision=precision)
    out = P.run_hip_forward(dyn, inp, z, t)
    assert torch.isfinite(out).all()
    ev, eh = errors(f'ties {graph} {precision}, fp64 oracle', out, LC.pocket_oracle_forward(case), z)
    assert ev <= tol and eh <= tol, (ev, eh)
    ev, eh = P.report(f'ties {graph} {precision}, reference fixture', out, torch.from_numpy(LC.fixture()[f'pocket.{graph}.out']), z)
    assert ev <= tol and eh <= tol, (ev, eh)
    assert torch.equal(P.run_hip_forward(dyn, inp, z, t), out), 'bitwise repeatable'
    for b in range(z.shape[0]):
        one = P.run_hip_forward(dyn, IC.alone(inp, b), z[b:b + 1], t[b:b + 1])
        assert torch.equal(one[0], out[b]), f'molecule {b} alone against its row of the batch'
    back = P.run_hip_forward(dyn, IC.reversed_batch(inp), z.flip(0), t.flip(0))
    assert torch.equal(back.flip(0), out), 'the batch reversed'


@pytest.mark.parametrize('graph', ['FC-10A-4A', 'FC-4A'])
def test_pocket_backward_at_the_ties(graph):
    case = LC.lattice_pocket_case(graph)
    inp, z, t = case.inp, case.z, case.t
    G = LC.cotangent(case)
    dyn = PT.make_dyn(LC.NF, 2, LC.POCKET_WEIGHTS['n_layers'], 2, wseed=LC.POCKET_WEIGHTS['seed'], graph_type=graph)
    ref = LC.pocket_oracle_grads(case, G)
    f32 = LC.pocket_oracle_grads(case, G, dtype=torch.float32)
    hip = PT.hip_grads(dyn, t, z, inp, G)
    assert set(hip) == set(ref) and all(torch.isfinite(v).all() for v in hip.values())
    total, worst = PT.compare(hip, ref)
    total32, worst32 = PT.compare(f32, ref)
    print(f'ties {graph}: rel-L2 all {total:.2e}, worst tensor {worst:.2e}; fp32 eager autograd {total32:.2e}, {worst32:.2e}')
    assert total <= PT.BAR_ALL and worst <= PT.BAR_TENSOR, (total, worst)
    assert total <= PT.FP32_CLASS * total32 and worst <= PT.FP32_CLASS * worst32, (total, total32, worst, worst32)
    again = PT.hip_grads(dyn, t, z, inp, G)
    assert all(torch.equal(hip[k], again[k]) for k in hip)
    # the forward of the training path is the inference forward (the same bits); the backward rebuilds the graph with its own
    # copy of the predicate, which the gradient comparison above pins
    g = {k: v.to(DEV) for k, v in inp.items()}
    with torch.no_grad():
        want = dyn.forward(t.to(DEV), z.to(DEV), g['node_mask'], g['linker_mask'], g['edge_mask'], g['context'])
    got = dyn.training_forward(t.to(DEV), z.to(DEV), g['node_mask'], g['linker_mask'], g['edge_mask'], g['context'])
    assert got.requires_grad and torch.equal(got.detach(), want)


# ---- bonds --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('is_geom', [False, True])
def test_bonds_at_the_thresholds(is_geom):
    from difflinker_amd import const
    from difflinker_amd.metrics import molecule_keys
    from difflinker_amd.molecule_builder import build_xae_molecules, is_connected, perceive_bonds
    from test_gpu_bonds import every_pair, expected
    case = LC.lattice_bond_molecules(is_geom)
    E_all = LC.fixture()[f'bonds.{"geom" if is_geom else "zinc"}.E'].astype(np.int64)
    one_hot, x, mask = case.one_hot, case.x, case.mask
    B, N = mask.shape[:2]
    dev = [v.to(DEV) for v in (one_hot, x, mask)]
    cap = every_pair(int(mask.sum(1).max()))
    found = perceive_bonds(*dev, is_geom, capacity=cap)
    one_piece = is_connected(*dev, is_geom).cpu()
    xae = build_xae_molecules(*dev, is_geom)
    keys = molecule_keys(dev[0], dev[2], found, is_geom)
    limits = const.max_valence_table(is_geom).tolist()
    # the same molecules with the junk rows removed, real rows packed to the front
    n_max = int(mask.sum(1).max())
    h3, x3, m3 = torch.zeros(B, n_max, one_hot.shape[2]), torch.zeros(B, n_max, 3), torch.zeros(B, n_max, 1)
    for b in range(B):
        keep = mask[b, :, 0] != 0
        n = int(keep.sum())
        h3[b, :n], x3[b, :n], m3[b, :n] = one_hot[b][keep], x[b][keep], 1
    packed = perceive_bonds(h3.to(DEV), x3.to(DEV), m3.to(DEV), is_geom, capacity=cap)
    for b, (name, kinds, pos) in enumerate(case.mols):
        n = len(kinds)
        rows, valence, labels = expected(E_all[b], n)
        assert int(found.n_bonds[b]) == len(rows), name
        assert found.bonds[b, :len(rows)].cpu().tolist() == [list(r) for r in rows], f'{name}: bond list, orders or their order'
        assert found.valence[b].cpu().tolist() == valence + [0] * (N - n), name
        assert found.component[b].cpu().tolist() == labels + [-1] * (N - n), name
        assert int(found.n_components[b]) == len(set(labels)) == LC.pieces(E_all[b][:n, :n]), name
        assert bool(one_piece[b]) == (len(set(labels)) == 1), name
        assert int(found.status[b]) == 0, name
        X, A, E = xae[b]
        assert X.tolist() == kinds.tolist() and np.array_equal(E.numpy(), E_all[b][:n, :n]) and torch.equal(A, E.bool()), name
        # what dl_molecule_keys derives from the list
        assert int(keys.n_atoms[b]) == n and int(keys.n_bonds[b]) == len(rows) and int(keys.status[b]) == 0, name
        assert int(keys.n_over[b]) == sum(v > limits[k] for v, k in zip(valence, kinds.tolist())), name
        assert int(keys.n_components[b]) == len(set(labels)), name
        # junk rows change nothing
        assert int(packed.n_bonds[b]) == len(rows) and torch.equal(packed.bonds[b, :len(rows)], found.bonds[b, :len(rows)]), name
        assert torch.equal(packed.valence[b, :n], found.valence[b, :n]) and int(packed.n_components[b]) == len(set(labels)), name
        if name.startswith('split'):
            assert int(found.n_components[b]) == 2, f'{name}: the O-N pair at exactly 1.5 A is not a bond'


# ---- size predictor -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', list(LC.SIZE_MODELS))
def test_size_gnn_at_the_filter(tag):
    case = LC.lattice_size_case()
    fix = LC.fixture()
    data = case.data
    L, bn = LC.SIZE_MODELS[tag]
    clf, sd = SG.make_classifier(LC.SIZE_IN_NF, LC.SIZE_OUT_NF, L, 500 + L, bn)
    dev = SG.to_dev(data)
    out, _ = clf.forward(dev, return_loss=False)
    out = out.cpu()
    refs = {'fp64 oracle': LC.size_logits(case, tag),
            'size_oracle': size_oracle.size_classifier_logits(sd, data['one_hot'], data['positions'], data['fragment_mask'],
                                                              data['edge_mask'], L, batch_norm=bn),
            'reference fixture': torch.from_numpy(fix[f'size.logits_{tag}'])}
    for name, ref in refs.items():
        err = rel_l2(out, ref)
        print(f'[size ties {tag}] positions, {name}: rel-L2 {err:.3e}')
        assert err <= SG.TOL, name
    # the precomputed-distances entry: the caller's filter (linker_size_lightning.py:107) on distances one step beside 6
    B, N = data['positions'].shape[:2]
    final = (data['edge_mask'].view(B, N, N).bool() & (case.distances < 6)).float()
    given = clf.gnn._launch(dev['one_hot'], dev['positions'], dev['fragment_mask'], final.to(DEV), case.distances.to(DEV)).cpu()
    for name, ref in (('fp64 oracle', LC.size_logits(case, tag, distances=case.distances)),
                      ('reference fixture', torch.from_numpy(fix[f'size.logits_given_{tag}']))):
        err = rel_l2(given, ref)
        print(f'[size ties {tag}] given distances, {name}: rel-L2 {err:.3e}')
        assert err <= SG.TOL, name


@pytest.mark.parametrize('tag', list(LC.SIZE_MODELS))
def test_size_gnn_training_at_the_filter(tag):
    case = LC.lattice_size_case()
    data = case.data
    L, bn = LC.SIZE_MODELS[tag]
    clf, sd = ST.make_clf(L, bn, seed=500 + L)
    ref_out, ref_loss, ref_g, _ = ST.ref_run(sd, data, L, bn)
    out, loss, g = ST.hip_run(clf, data)
    err = rel_l2(out, ref_out)
    overall, worst, zeros = ST.compare(g, ref_g, bn)
    print(f'[size ties {tag}] training logits rel-L2 {err:.3e}; grad all {overall:.3e}, worst tensor {worst:.3e}, '
          f'pre-BN biases {zeros:.1e}')
    assert err <= 1e-5 and abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    assert overall <= ST.BAR_ALL and worst <= ST.BAR_TENSOR and zeros <= 1e-5
    if not bn:                                  # without BatchNorm the training forward computes what inference computes
        infer, _ = clf.eval().forward(ST.to_dev(data), return_loss=False)
        assert rel_l2(out, infer.cpu()) <= SG.TOL
        assert rel_l2(out, torch.from_numpy(LC.fixture()[f'size.logits_{tag}'])) <= SG.TOL


# ---- coincident atoms on the fully-connected graph -----------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('name', list(LC.FC_COINCIDENT))
def test_coincident_atoms_forward(name, precision):
    inp, z, t = LC.fc_coincident_case(name)
    dyn, _, _ = P.make_dynamics(LC.FC_NF, 1, LC.FC_WEIGHTS['n_layers'], seed=LC.FC_WEIGHTS['seed'], precision=precision)
    out = P.run_hip_forward(dyn, inp, z, t)                      # (a raised FoundNaNException is a set flag)
    assert torch.isfinite(out).all()
    for tag, ref in (('fp64 oracle', errors), ('fp32 oracle', P.report)):
        dtype = torch.float64 if ref is errors else torch.float32
        ev, eh = ref(f'coincident {name} {precision}, {tag}', out, LC.fc_oracle(name, dtype=dtype), z)
        assert ev <= P.FWD_TOLS[precision] and eh <= P.FWD_TOLS[precision], (tag, ev, eh)


@pytest.mark.parametrize('name', list(LC.FC_COINCIDENT))
def test_coincident_atoms_backward(name):
    inp, z, t = LC.fc_coincident_case(name)
    G = torch.randn(z.shape, generator=torch.Generator().manual_seed(3))
    dyn = FT.make_dyn(LC.FC_NF, 1, LC.FC_WEIGHTS['n_layers'], 2, wseed=LC.FC_WEIGHTS['seed'])
    _, ref = LC.fc_oracle(name, G)
    hip = FT.hip_grads(dyn, t, z, inp['node_mask'], inp['linker_mask'], inp['edge_mask'], inp['context'], G)
    assert set(hip) == set(ref) and all(torch.isfinite(v).all() for v in hip.values())
    total, worst = FT.compare(hip, ref)
    print(f'coincident {name}: rel-L2 all {total:.2e}, worst tensor {worst:.2e}')
    assert total <= FT.BAR_ALL and worst <= FT.BAR_TENSOR, (total, worst)
