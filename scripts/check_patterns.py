"""Compile status of every row of a pattern file under difflinker_amd/patterns.py: `python scripts/check_patterns.py FILE`
(or `basic`).  One line per row (`ok` with the number of pattern atoms after the hydrogen merge and of sub-patterns it uses,
or the construct that is not supported and its column), then a summary.  `--summary` prints the summary alone, which names
rows and constructs but no SMARTS text."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from difflinker_amd import patterns as P        # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('file')
p.add_argument('--summary', action='store_true')
a = p.parse_args()
rows = P.read_pattern_file(P.basic_catalogue_path() if a.file == 'basic' else a.file)
accepted, rejected, largest, recursive = [], [], 0, 0
for k, row in enumerate(rows):
    try:
        one = P.compile_patterns([row])
    except P.PatternError as e:
        rejected.append((k, row[1], e.construct, e.column))
        if not a.summary:
            print(f'{k}\t{row[1]}\trejected: {e.construct} at column {e.column}')
        continue
    accepted.append(row)
    atoms = int(one.pat[one.n_sub, 1])
    largest, recursive = max(largest, atoms), recursive + (one.n_sub > 0)
    if not a.summary:
        print(f'{k}\t{row[1]}\tok: {atoms} atoms, {one.n_sub} sub-patterns')
print(f'rows: {len(rows)}  accepted: {len(accepted)}  rejected: {len(rejected)}')
for k, name, construct, column in rejected:
    print(f'  rejected row {k} ({name}): {construct} at column {column}')
if accepted:
    whole = P.compile_patterns(accepted)
    print(f'largest pattern: {largest} atoms (limit {P.MAX_PATTERN_ATOMS});  rows with $(...): {recursive};  distinct '
          f'sub-patterns: {whole.n_sub} (limit {P.MAX_SUBPATTERNS});  nesting levels: {len(whole.level_end)} (limit '
          f'{P.MAX_LEVELS});  longest predicate: {int(whole.atoms[:, 3].max())} tokens (limit {P.MAX_PRED});  table rows: '
          f'{whole.atoms.shape[0]} atoms, {whole.closures.shape[0]} closures, {whole.preds.numel()} tokens')
