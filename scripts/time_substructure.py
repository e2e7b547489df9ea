"""Time of one dl_substructure_match launch, with one dl_pharmacophore_features launch on the same batch beside it for scale:
device events around back-to-back calls, after a warm-up.  The benchmark's batch shape: B = 256 molecule-like graphs of 35..50
atoms on N = 50 rows (tests/substructure_cases.random_molecule), a third of the atoms marked, handed over as a bond list with
aromatic flags.  Two catalogues: `basic` (difflinker_amd/data/filters_basic.csv) and 480 synthetic patterns of 1..12 atoms cut
out of such molecules by the test generator (tests/substructure_cases.random_pattern); --patterns FILE times a pattern file.
--stats M also runs the restatement (tests/substructure_ref.py) on the first M molecules on the CPU and reports the steps per
searched root and the share of (molecule, pattern) pairs the element screen and the size test remove; --stats_only skips the
GPU."""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import substructure_cases as sc                 # noqa: E402
import substructure_ref as sr                   # noqa: E402
from difflinker_amd import patterns as P        # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--calls', type=int, default=20)
p.add_argument('--repeats', type=int, default=5)
p.add_argument('--max_steps', type=int, default=4096)
p.add_argument('--patterns', default=None)
p.add_argument('--stats', type=int, default=0)
p.add_argument('--stats_only', action='store_true')
a = p.parse_args()
B, N = 256, 50
rng = random.Random(3)
drawn = []
while len(drawn) < B:                           # (a molecule whose valences fill up early stays small: drawn again)
    m = sc.random_molecule(rng, N, 35)
    if len(m[0]) >= 35:
        drawn.append(m)
marks = [[random.Random(b * 31 + k).random() < 1 / 3 for k in range(len(m[0]))] for b, m in enumerate(drawn)]


def restated(m, marked=None):
    return sr.Molecule([sc.NUMBER[s] for s in m[0]], [sc.VALENCE[s] for s in m[0]], m[1], [k in m[2] for k in range(len(m[1]))],
                       marked=marked)


def synthetic(n_patterns=480):
    source = [restated(m) for m in drawn[:64]]
    out = []
    while len(out) < n_patterns:
        mol = rng.choice(source)
        size = rng.choice([1, 2, 2, 3, 3, 4, 4, 5, 6, 7, 8, 10, 12])
        out.append(sc.random_pattern(rng, mol, size, rng.choice([0.2, 0.5, 0.8]), rng.choice([0, 0, 0, 0, 0, 0, 0, 1, 1, 2])))
    return out


catalogues = {'basic': P.load_catalogue('basic'), 'synthetic 480': P.compile_patterns(synthetic())}
if a.patterns:
    catalogues[os.path.basename(a.patterns)] = P.load_catalogue(a.patterns)
sizes = [len(m[0]) for m in drawn]
print('B = %d, N = %d: atoms per molecule %.1f (min %d, max %d), bonds per molecule %.1f, aromatic bonds %.1f' % (
    B, N, np.mean(sizes), min(sizes), max(sizes), np.mean([len(m[1]) for m in drawn]), np.mean([len(m[2]) for m in drawn])))
for name, catalogue in catalogues.items():
    print('%s: %d patterns, %d sub-patterns in %d levels, largest pattern %d atoms' % (
        name, catalogue.n_top, catalogue.n_sub, len(catalogue.level_end), int(catalogue.pat[catalogue.n_sub:, 1].max())))
    if a.stats:
        matcher, steps, screened, hits, budget = sr.Matcher(catalogue), [], 0, 0, 0
        for b in range(a.stats):
            out = matcher.match(restated(drawn[b], marks[b]), max_steps=a.max_steps, with_marks=True)
            steps += list(out['steps'].values())
            screened, hits, budget = screened + out['screened'], hits + out['n_hits'], budget + bool(out['status'] & sr.BUDGET)
        pairs = a.stats * catalogue.n_top
        print('  restatement on %d molecules: %.1f%% of the pairs removed before any search, %.1f%% of the pairs hit; steps per '
              'searched root mean %.2f, median %d, 99th percentile %d, max %d; molecules with the budget bit at max_steps %d: %d' % (
                  a.stats, 100 * screened / pairs, 100 * hits / pairs, np.mean(steps), np.median(steps), np.percentile(steps, 99),
                  max(steps), a.max_steps, budget))
if a.stats_only:
    sys.exit(0)

import torch                                    # noqa: E402
from difflinker_amd import _lib, metrics        # noqa: E402

DEV = 'cuda:0'
batch = sc.batch_of([sc.molecule(*m, marked=marks[b]) for b, m in enumerate(drawn)], N, scatter=False)
one_hot, mask, drop, mark, found, flags = batch
one_hot, mask, mark, flags = one_hot.to(DEV), mask.to(DEV), mark.to(DEV), flags.to(DEV)
found = sc.on_device(found, lambda t: t.to(DEV))
x = torch.randn(B, N, 3, device=DEV) * 3


def pharm():
    return metrics.pharmacophore_features(one_hot, x, mask, found, flags, True, mark_mask=mark)


def match(catalogue):
    return metrics.match_patterns(one_hot, x, mask, found, flags, catalogue, True, mark_mask=mark, max_steps=a.max_steps)


calls = [('dl_pharmacophore_features', pharm)] + [(f'dl_substructure_match, {name}', lambda c=c: match(c)) for name, c in catalogues.items()]
for name, call in calls:
    for _ in range(3):
        out = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.calls):
            call()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / a.calls)
    print('%s: milliseconds per call over %d back-to-back calls, %d repeats: %s; median %.3f' % (
        name, a.calls, a.repeats, ' '.join('%.3f' % v for v in times), float(np.median(times))))
    if hasattr(out, 'n_hits'):
        print('  hits per molecule %.2f, through a marked atom %.2f; molecules with DL_SUB_BUDGET %d, with any other bit %d' % (
            float(out.n_hits.float().mean()), float(out.n_hits_marked.float().mean()),
            int(((out.status & _lib.DL_SUB_BUDGET) != 0).sum()), int(((out.status & ~_lib.DL_SUB_BUDGET) != 0).sum())))
print('device:', torch.cuda.get_device_name(0))
