"""fp64 restatement of ``SizeClassifier.forward`` in TRAINING mode (linker_size_lightning.py:83-117): the oracle's GCL
(oracle/size_oracle.py) with ``nn.BatchNorm1d`` normalising over all ``B*N`` rows (biased variance, eps 1e-5).  Used by the
size-predictor training tests as the autograd reference."""
import torch
import torch.nn.functional as F

from oracle.egnn_oracle import coord2diff, fc_edges, segment_sum

ZINC_SIZES = list(range(3, 13))


def _lin(p, key, x):
    return F.linear(x, p[key + '.weight'], p.get(key + '.bias'))


def _bn_train(p, key, x, stats, eps=1e-5):
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    stats[key] = (mean.detach(), var.detach())
    return (x - mean) / torch.sqrt(var + eps) * p[key + '.weight'] + p[key + '.bias']


def _gcl(p, pre, h, row, col, edge_attr, node_mask, edge_mask, batch_norm, stats):
    m = F.relu(_lin(p, pre + '.edge_mlp.0', torch.cat([h[row], h[col], edge_attr], dim=1)))
    m = F.relu(_lin(p, pre + '.edge_mlp.2', m)) * edge_mask
    t = torch.cat([h, segment_sum(m, row, h.size(0), 1.0)], dim=1)
    if batch_norm:
        t = F.relu(_bn_train(p, pre + '.node_mlp.1', _lin(p, pre + '.node_mlp.0', t), stats))
        out = _bn_train(p, pre + '.node_mlp.4', _lin(p, pre + '.node_mlp.3', t), stats)
    else:
        out = _lin(p, pre + '.node_mlp.2', F.relu(_lin(p, pre + '.node_mlp.0', t)))
    return (h + out) * node_mask


def train_logits(p, one_hot, positions, fragment_mask, edge_mask, n_layers, batch_norm, pre='gnn.'):
    """Returns (logits [B, out], {bn key: (batch mean, biased batch var)}); p: state_dict-keyed tensors (fp64, leaves)."""
    bs, n = positions.shape[:2]
    fm = fragment_mask.reshape(bs, n, 1).to(positions.dtype)
    x = (positions * fm).reshape(bs * n, -1)
    h = (one_hot * fm).reshape(bs * n, -1)
    row, col = fc_edges(n, bs)
    distances, _ = coord2diff(x, row, col)
    dmask = (edge_mask.reshape(-1, 1).bool() & (distances < 6)).to(h.dtype)
    stats = {}
    h = _lin(p, pre + 'embedding_in', h)
    keys = [pre + 'gcl1'] + [pre + f'gcl_layers.{i}' for i in range(n_layers - 1)]
    for key in keys:
        h = _gcl(p, key, h, row, col, distances, fm.reshape(bs * n, 1), dmask, batch_norm, stats)
    out = _lin(p, pre + 'embedding_out', h)
    return out.view(bs, n, -1).mean(1), stats


def true_labels(linker_mask, sizes=ZINC_SIZES):
    """``get_true_labels`` with the ZINC table: unseen sizes map to the largest class."""
    size2id = {s: i for i, s in enumerate(sizes)}
    n = linker_mask.reshape(linker_mask.shape[0], -1).sum(-1).long().tolist()
    return torch.tensor([size2id.get(int(s), size2id[max(sizes)]) for s in n], dtype=torch.long)


def size_batch(sizes, linkers, in_nf, seed, scale=1.6, chain=False):
    """A ``collate_with_fragment_edges`` batch of random molecules (fragments first, linker atoms last).  ``chain``: positions
    are a random walk of step ``scale`` (a few kept edges per atom, as in real molecules) instead of a Gaussian cloud."""
    from difflinker_amd.datasets import collate_with_fragment_edges
    g = torch.Generator().manual_seed(seed)
    mols = []
    for n, nl in zip(sizes, linkers):
        frag = torch.zeros(n)
        frag[:n - nl] = 1
        types = torch.randint(0, in_nf, (n,), generator=g)
        pos = scale * torch.randn((n, 3), generator=g)
        mols.append({'positions': torch.cumsum(pos, 0) if chain else pos,
                     'one_hot': torch.nn.functional.one_hot(types, in_nf).float(), 'anchors': torch.zeros(n),
                     'fragment_mask': frag, 'linker_mask': 1 - frag, 'num_atoms': n, 'uuid': 0, 'name': 'm'})
    return collate_with_fragment_edges(mols)
