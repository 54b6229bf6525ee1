"""Recorded results of the reference's precision / recall.  AUTHORING ONLY: needs the reference checkout.

    python tools/make_pr_goldens.py      -> tests/golden/pr_ref.npz

Loads metrics/sid_precision_recall.py of the reference FROM ITS FILE with a stub `sid_metric_utils` whose two feature functions
return the fixture's features (tests/test_pr_host.py::pr_fixture: regenerated from the seed, never stored), and calls the UNMODIFIED
`compute_pr` (and through it `compute_distances`) on the CPU.  Stored per case (seed, n_real, n_gen): precision, recall, and -- by
running the same two reference functions once more the way compute_pr does -- the fp16 radii and the per-probe decisions.  Only
results and parameters are stored.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from oracle import ref_harness  # noqa: E402
from test_pr_host import PR_CASES, PR_F, PR_K, pr_fixture  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'pr_ref.npz')
ROW_BATCH, COL_BATCH = 10000, 10000         # the reference's own (sid_metric_main.py: pr50k3_full)


class _Stats:
    def __init__(self, x):
        self.x = x

    def get_all_torch(self):
        return torch.from_numpy(self.x)


def load_reference(ref_dir, features):
    """The reference module, its `from . import sid_metric_utils` resolved to a stub that hands out `features`."""
    pkg = types.ModuleType('refmetrics')
    pkg.__path__ = [os.path.join(ref_dir, 'metrics')]
    stub = types.ModuleType('refmetrics.sid_metric_utils')
    stub.compute_feature_stats_for_dataset = lambda **kw: _Stats(features['real'][:kw.get('max_items')])
    stub.compute_feature_stats_for_generator = lambda **kw: _Stats(features['gen'][:kw.get('max_items')])
    sys.modules['refmetrics'], sys.modules['refmetrics.sid_metric_utils'] = pkg, stub
    spec = importlib.util.spec_from_file_location('refmetrics.sid_precision_recall', os.path.join(ref_dir, 'metrics', 'sid_precision_recall.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    assert ref_harness.reference_available(), f'{ref_harness.REFERENCE_ROOT} not present'
    ref_dir = ref_harness.REFERENCE_ROOT
    features = {}
    ref = load_reference(ref_dir, features)
    opts = types.SimpleNamespace(num_gpus=1, rank=0, device=torch.device('cpu'))
    out = dict(F=np.int64(PR_F), k=np.int64(PR_K), cases=np.array(PR_CASES, dtype=np.int64), row_batch=np.int64(ROW_BATCH),
               col_batch=np.int64(COL_BATCH))
    for seed, n_real, n_gen in PR_CASES:
        features['real'], features['gen'] = pr_fixture(seed, n_real, n_gen)
        tag = f'{seed}_{n_real}_{n_gen}'
        precision, recall = ref.compute_pr(opts, max_real=None, num_gen=n_gen, nhood_size=PR_K, row_batch_size=ROW_BATCH, col_batch_size=COL_BATCH)
        out[f'precision_{tag}'], out[f'recall_{tag}'] = np.float64(precision), np.float64(recall)
        real16, gen16 = (torch.from_numpy(features[n]).to(torch.float16) for n in ('real', 'gen'))
        for name, manifold, probes in (('precision', real16, gen16), ('recall', gen16, real16)):
            dist = ref.compute_distances(row_features=manifold, col_features=manifold, num_gpus=1, rank=0, col_batch_size=COL_BATCH)
            radius = dist.to(torch.float32).kthvalue(PR_K + 1).values.to(torch.float16)
            dist = ref.compute_distances(row_features=probes, col_features=manifold, num_gpus=1, rank=0, col_batch_size=COL_BATCH)
            inside = (dist <= radius).any(dim=1)
            assert abs(float(inside.to(torch.float32).mean()) - out[f'{name}_{tag}']) < 1e-7
            out[f'{name}_radius_{tag}'] = radius.numpy()
            out[f'{name}_inside_{tag}'] = inside.numpy()
        print(tag, f'precision {precision:.4f} recall {recall:.4f}')
    np.savez_compressed(OUT, **out)
    print(OUT, f'{os.path.getsize(OUT) / 1e3:.0f} kB')


if __name__ == '__main__':
    main()
