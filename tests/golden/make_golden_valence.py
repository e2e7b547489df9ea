"""Generate ``valence_table.npz`` from the UNMODIFIED reference: ``ALLOWED_BONDS`` and both atom vocabularies of its
``src/const.py`` (:14, :29, :156-171).

Run in the build container only (it imports the reference, which does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_valence.py

RDKit is replaced by the stand-ins of ``make_golden._stub_reference_dependencies``.  The file holds data only and is written
with fixed zip time stamps, so a second run reproduces it bit for bit.

``elements``       the keys of ``ALLOWED_BONDS``; ``allowed`` ``[len(elements), 2]``: the alternatives of each element, padded
                   with -1 (an integer entry has one alternative, ``P: [3, 5]`` has two).
``zinc_symbols`` / ``geom_symbols``  the vocabularies in index order (``IDX2ATOM``, ``GEOM_IDX2ATOM``).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _stub_reference_dependencies      # noqa: E402  (sets sys.path: repository, tests/, reference)

_stub_reference_dependencies()
from src import const as ref_const                         # noqa: E402
from make_golden_bonds import save_deterministic           # noqa: E402


def tables():
    elements = list(ref_const.ALLOWED_BONDS)
    allowed = np.full((len(elements), 2), -1, np.int32)
    for k, el in enumerate(elements):
        v = ref_const.ALLOWED_BONDS[el]
        v = list(v) if isinstance(v, (list, tuple)) else [v]
        assert 1 <= len(v) <= 2
        allowed[k, :len(v)] = v
    vocab = lambda d: np.array([d[k] for k in range(len(d))])      # noqa: E731
    return {'elements': np.array(elements), 'allowed': allowed, 'zinc_symbols': vocab(ref_const.IDX2ATOM),
            'geom_symbols': vocab(ref_const.GEOM_IDX2ATOM)}


if __name__ == '__main__':
    save_deterministic('valence_table', tables())
