"""Host side of precision / recall and of the real-image path (no GPU): the image dataset, the real-set feature statistics, and the
fixture + fp64 restatement that tests/test_gpu_pr.py and tools/make_pr_goldens.py share."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------
# Fixture: features on a 6-dimensional manifold (isotropic high-dimensional noise makes all distances equal to within fp16 ulps).
#   A = randn(6, F) / sqrt(6);  b = 0.3 |randn(F)|;  x = max(z A + b + 0.01 randn(n, F), 0)
#   real: z = randn(n, 6);  generated: z = 0.8 randn(n, 6) + 0.35
PR_F, PR_K = 2048, 3
PR_CASES = [(seed, n_real, n_gen) for seed in (1, 2) for n_real, n_gen in ((416, 352), (1216, 1088))]


def pr_fixture(seed, n_real, n_gen, F=PR_F):
    """-> (real [n_real, F], gen [n_gen, F]) float32, the same bits everywhere (numpy.random.RandomState)."""
    rs = np.random.RandomState(seed)
    A = rs.randn(6, F) / np.sqrt(6.0)
    b = 0.3 * np.abs(rs.randn(F))
    z_real = rs.randn(n_real, 6)
    z_gen = 0.8 * rs.randn(n_gen, 6) + 0.35
    real = np.maximum(z_real @ A + b + 0.01 * rs.randn(n_real, F), 0.0)
    gen = np.maximum(z_gen @ A + b + 0.01 * rs.randn(n_gen, F), 0.0)
    return real.astype(np.float32), gen.astype(np.float32)


def pr_error_bound(F):
    """c with: |computed d2 - d2| <= c (|a|^2 + |b|^2) for the kernel's arithmetic (csrc/pr_dist.hip).
    Each of |a|^2, |b|^2 and a . b is a sum of F products of fp16 numbers -- exact in fp32 -- accumulated by a chain of F / 32
    MFMA instructions, each adding 32 products to the fp32 accumulator with an error of at most one fp32 ulp, 2^-23, of the
    partial sum.  Partial sums are bounded by sum |a_k b_k| <= (|a|^2 + |b|^2) / 2 (and by the norm itself for the norms), so the
    worst case over the three chains is (F / 32) 2^-23 (|a|^2 + |b|^2 + 2 sum |a_k b_k|) <= (F / 16) 2^-23 (|a|^2 + |b|^2), and the
    three roundings of (|a|^2 + |b|^2) - 2 a . b and the correctly rounded sqrt add less than 2^-21 (|a|^2 + |b|^2).  That worst
    case, every rounding at its maximum and in one direction, is not approached by round-to-nearest errors, which grow with the
    square root of the chain length; the bound used is the one the metric's specification was checked with,
        c = 4 sqrt(F) 2^-23,      i.e. relative to the distance  e = c (|a|^2 + |b|^2) / (2 d^2) = 2 sqrt(F) 2^-23 (|a|^2 + |b|^2) / d^2,
    which for F = 2048 (2.16e-5) still lies ABOVE that worst case ((128 + 4) 2^-23 = 1.57e-5).  It follows from the fp64 values and
    the kernel's accumulation lengths only, never from what the kernel returns."""
    c = 4.0 * np.sqrt(F) * 2.0 ** -23
    assert F > 4096 or c >= (F / 16 + 4) * 2.0 ** -23
    return c


def pr_restate(rows16, cols16):
    """fp64 restatement of the distance matrix between two fp16 feature sets (CPU tensors).  -> dict of [R, C] tensors:
    exact = fp16(d);  lo, hi = fp16(d (1 - e)), fp16(d (1 + e)) with the per-pair relative bound e of pr_error_bound;
    wide = e >= 1 (d is so small -- a row against itself or a duplicate -- that only 0 <= value <= hi = fp16(2 d) can be asked)."""
    a, b = rows16.double(), cols16.double()
    s = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]
    d2 = (s - 2.0 * (a @ b.t())).clamp_min(0.0)
    d = d2.sqrt()
    e = (0.5 * pr_error_bound(rows16.shape[1]) * s / d2.clamp_min(1e-300)).clamp_max(1.0)
    wide = e >= 1.0
    f16 = lambda t: t.to(torch.float16)        # noqa: E731  (round to nearest even, once)
    return dict(exact=f16(d), lo=f16(d * (1.0 - e)), hi=f16(d * (1.0 + e)), wide=wide)


def kth(dist16, k):
    """`dist.to(float32).kthvalue(k + 1).values.to(float16)` (metrics/sid_precision_recall.py:59)."""
    return dist16.to(torch.float32).kthvalue(k + 1).values.to(torch.float16)


def pr_restate_decisions(manifold16, probes16, k):
    """-> (inside [P] bool by the restatement, robust [P] bool, radius fp16 [N]).  kth is monotone in every distance, so the radius
    of a column lies between kth(lo) and kth(hi); a probe is robustly inside if some column has hi <= radius_lo, robustly outside if
    every column has lo > radius_hi, otherwise fragile."""
    mm = pr_restate(manifold16, manifold16)
    pm = pr_restate(probes16, manifold16)
    radius, radius_lo, radius_hi = kth(mm['exact'], k), kth(mm['lo'], k), kth(mm['hi'], k)
    inside = (pm['exact'] <= radius).any(1)
    robust_in = (pm['hi'] <= radius_lo).any(1)
    robust_out = (pm['lo'] > radius_hi).all(1)
    return inside, robust_in | robust_out, radius


def test_restatement_and_fixture_are_sane():
    """The fixture has the shape the checks assume: precision and recall away from 0 and 1, few fragile probes, and a boundary share
    below the cap of the element-wise check (computed on the CPU, no kernel involved)."""
    real, gen = (torch.from_numpy(x).to(torch.float16) for x in pr_fixture(1, 416, 352))
    inside, robust, radius = pr_restate_decisions(real, gen, PR_K)
    assert 0.9 < inside.float().mean() < 1.0 and (~robust).float().mean() <= 0.005
    inside_r, robust_r, _ = pr_restate_decisions(gen, real, PR_K)
    assert 0.5 < inside_r.float().mean() < 0.9 and (~robust_r).float().mean() <= 0.005
    r = pr_restate(gen, real)
    share = (r['lo'] != r['hi']).float().mean()
    print(f'boundary share {share:.4f}')
    assert share <= 0.10
    assert (r['lo'] <= r['exact']).all() and (r['exact'] <= r['hi']).all()
    assert pr_restate(real, real)['wide'].diagonal().all()


def test_pr_golden_is_consistent_with_the_restatement(golden_dir):
    """tests/golden/pr_ref.npz (the UNMODIFIED reference on the CPU, tools/make_pr_goldens.py) against the exact restatement: the
    recorded decisions differ on a few probes at most (here: 2 of 1 216 in one set, none in the other seven) -- the reference's fp16
    cdist is not correctly rounded, 60 % of its radii are an ulp off.  tests/test_gpu_pr.py counts these probes into its tolerance."""
    g = np.load(os.path.join(golden_dir, 'pr_ref.npz'))
    assert int(g['F']) == PR_F and int(g['k']) == PR_K and [tuple(c) for c in g['cases']] == PR_CASES
    for seed, n_real, n_gen in PR_CASES:
        real, gen = (torch.from_numpy(x).to(torch.float16) for x in pr_fixture(seed, n_real, n_gen))
        tag = f'{seed}_{n_real}_{n_gen}'
        for name, manifold, probes in (('precision', real, gen), ('recall', gen, real)):
            inside, _, _ = pr_restate_decisions(manifold, probes, PR_K)
            rec = torch.from_numpy(g[f'{name}_inside_{tag}'])
            assert abs(float(g[f'{name}_{tag}']) - float(rec.float().mean())) < 1e-6
            differ = int((rec != inside).sum())
            print(f'{tag} {name}: reference != restatement on {differ} of {len(rec)} probes')
            assert differ <= 0.005 * len(rec)


# ------------------------------------------------------------------------------------------------
def _write_images(root):
    """A small image folder: RGB, grey, RGBA, a nested folder, an image without caption, a caption without image."""
    import PIL.Image
    rs = np.random.RandomState(5)
    pix = {}

    def put(rel, mode, caption, size=(12, 8)):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        w, h = size
        shape = {'RGB': (h, w, 3), 'L': (h, w), 'RGBA': (h, w, 4)}[mode]
        arr = rs.randint(0, 256, shape).astype(np.uint8)
        PIL.Image.fromarray(arr, mode).save(path)
        if caption is not None:
            with open(os.path.splitext(path)[0] + '.txt', 'wt') as f:
                f.write(caption + '\n')
        pix[rel] = arr
    put('b_rgb.png', 'RGB', 'a red bus')
    put('a_grey.png', 'L', '  a grey cat ')
    put('c_rgba.png', 'RGBA', 'a clear glass')
    put('sub/d_nested.png', 'RGB', 'a nested dog')
    put('e_uncaptioned.png', 'RGB', None)
    with open(os.path.join(root, 'f_no_image.txt'), 'wt') as f:
        f.write('a caption without image\n')
    return pix


def test_image_caption_dataset(tmp_path):
    """training/mscoco_dataset.py:11-68: sorted recursive walk, captioned images only, convert('RGB'), uint8 [3, H, W], stripped
    captions; the same captions in the same order as CaptionDataset."""
    import PIL.Image
    from sid_lsg_amd.data import CaptionDataset, ImageCaptionDataset, has_image_files
    pix = _write_images(str(tmp_path))
    ds = ImageCaptionDataset(str(tmp_path), resolution=64)
    order = ['a_grey.png', 'b_rgb.png', 'c_rgba.png', 'sub/d_nested.png']
    assert len(ds) == 4 and [os.path.relpath(f[0], str(tmp_path)) for f in ds.files] == order
    assert [ds[i][1] for i in range(4)] == ['a grey cat', 'a red bus', 'a clear glass', 'a nested dog']
    caps = CaptionDataset(str(tmp_path), resolution=64)
    assert [caps[i][1] for i in range(len(caps))] == [ds[i][1] for i in range(4)] == [ds.caption(i) for i in range(4)]
    for i, rel in enumerate(order):
        img = ds[i][0]
        assert img.dtype == torch.uint8 and tuple(img.shape) == (3, 8, 12)
        want = np.asarray(PIL.Image.open(os.path.join(str(tmp_path), rel)).convert('RGB')).transpose(2, 0, 1)
        assert (img.numpy() == want).all()
    assert (ds[1][0].numpy() == pix['b_rgb.png'].transpose(2, 0, 1)).all()
    assert (ds[0][0].numpy() == np.stack([pix['a_grey.png']] * 3)).all()
    assert (ds[2][0].numpy() == pix['c_rgba.png'][..., :3].transpose(2, 0, 1)).all()
    flipped = ImageCaptionDataset(str(tmp_path), resolution=64, random_flip=1.0)
    assert (flipped[1][0].numpy() == pix['b_rgb.png'][:, ::-1].transpose(2, 0, 1)).all() and flipped[1][1] == 'a red bus'
    assert has_image_files(str(tmp_path)) and not has_image_files(str(tmp_path / 'f_no_image.txt'))
    with pytest.raises(IOError):
        ImageCaptionDataset(str(tmp_path / 'f_no_image.txt'))


def _detector(images, return_features=True):
    """uint8 NCHW -> [N, 5] features: channel means and two fixed mixtures (needs 3 channels)."""
    x = images.to(torch.float64)
    m = x.mean(dim=(2, 3))
    return torch.cat([m, (x[:, 0] * x[:, 1]).mean(dim=(1, 2))[:, None] / 255.0, x[:, 2, ::2].std(dim=(1, 2))[:, None]], 1).to(torch.float32)


def _features_numpy(root):
    from sid_lsg_amd.data import ImageCaptionDataset
    ds = ImageCaptionDataset(root)
    return np.stack([_detector(ds[i][0][None])[0].numpy() for i in range(len(ds))]).astype(np.float64)


def test_dataset_feature_stats_matches_numpy(tmp_path):
    from sid_lsg_amd import metrics
    from sid_lsg_amd.data import CaptionDataset, ImageCaptionDataset
    _write_images(str(tmp_path))
    opts = metrics.MetricOptions(G=None, dataset=ImageCaptionDataset(str(tmp_path)), detector=_detector, device='cpu')
    feats = _features_numpy(str(tmp_path))
    mu, sigma = metrics.dataset_feature_stats(opts).get_mean_cov()
    assert np.abs(mu - feats.mean(0)).max() <= 1e-12 * np.abs(feats).max()
    assert np.abs(sigma - np.cov(feats, rowvar=False, bias=True)).max() <= 1e-12 * np.abs(feats).max() ** 2
    allf = metrics.dataset_feature_stats(opts, capture_all=True).get_all_torch()
    assert allf.dtype == torch.float32 and (allf.numpy() == feats.astype(np.float32)).all()
    three = metrics.dataset_feature_stats(opts, max_items=3, capture_all=True).get_all_torch()
    assert (three == allf[:3]).all()
    # the cache: computed once into <run_dir>/real_stats.npz, reloaded from there, and a valid --data_stat file
    opts.run_dir = str(tmp_path / 'run')
    mu1, sigma1 = metrics.load_real_stats(None, opts)
    cache = os.path.join(opts.run_dir, 'real_stats.npz')
    assert os.path.isfile(cache) and (mu1 == mu).all() and (sigma1 == sigma).all()
    opts.detector = None            # a second call must not need the detector
    mu2, sigma2 = metrics.load_real_stats(None, opts)
    mu3, sigma3 = metrics.load_real_stats(cache)
    assert (mu2 == mu).all() and (sigma3 == sigma).all() and (mu3 == mu).all() and (sigma2 == sigma).all()
    with pytest.raises(ValueError):
        metrics.dataset_feature_stats(metrics.MetricOptions(G=None, dataset=CaptionDataset(str(tmp_path)), detector=_detector, device='cpu'))
    with pytest.raises(ValueError):
        metrics.load_real_stats(None, metrics.MetricOptions(G=None, prompts=['x'], detector=_detector, device='cpu'))


def test_dataset_feature_stats_two_ranks(tmp_path):
    """Two gloo ranks: each takes every second image; after the merge both hold the single-process result."""
    from sid_lsg_amd import metrics
    from sid_lsg_amd.data import ImageCaptionDataset
    root, out = str(tmp_path / 'img'), str(tmp_path)
    _write_images(root)
    script = tmp_path / 'w.py'
    script.write_text(f'''
import os, sys
import numpy as np
sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]
from sid_lsg_amd import distributed as dist, metrics
from sid_lsg_amd.data import ImageCaptionDataset
from test_pr_host import _detector
dist.init(backend="gloo")
opts = metrics.MetricOptions(G=None, dataset=ImageCaptionDataset({root!r}), detector=_detector, device="cpu")
assert opts.num_gpus == 2 and opts.rank == dist.get_rank()
mu, sigma = metrics.dataset_feature_stats(opts).get_mean_cov()
allf = metrics.dataset_feature_stats(opts, capture_all=True).get_all_torch().numpy()
np.savez(os.path.join({out!r}, f"rank{{opts.rank}}.npz"), mu=mu, sigma=sigma, allf=allf)
''')
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', MASTER_ADDR='127.0.0.1')       # the CPU path, on a GPU host too
    run = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                          '127.0.0.1', '--master-port', '29637', str(script)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    opts = metrics.MetricOptions(G=None, dataset=ImageCaptionDataset(root), detector=_detector, device='cpu')
    mu, sigma = metrics.dataset_feature_stats(opts).get_mean_cov()
    allf = metrics.dataset_feature_stats(opts, capture_all=True).get_all_torch().numpy()
    for rank in (0, 1):
        r = np.load(os.path.join(out, f'rank{rank}.npz'))
        assert (r['allf'] == allf).all()
        assert np.abs(r['mu'] - mu).max() <= 1e-12 * np.abs(allf).max()
        assert np.abs(r['sigma'] - sigma).max() <= 1e-12 * np.abs(allf).max() ** 2


def test_pr_metrics_are_registered():
    from sid_lsg_amd import metrics
    assert metrics.is_valid_metric('pr30k3_full') and metrics.is_valid_metric('pr_test')
    assert metrics.list_valid_metrics()[:4] == ['fid30k_full', 'fid_clip_30k_full', 'fid_test', 'fid_clip_test']
