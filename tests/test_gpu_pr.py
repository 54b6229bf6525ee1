"""Precision / recall on the GPU: the sidlsg_pr_* kernels against the fp64 restatement of tests/test_pr_host.py, against each other,
and metrics.compute_pr against the recorded results of the reference (tests/golden/pr_ref.npz); the command line end to end."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from test_pr_host import PR_CASES, PR_K, kth, pr_fixture, pr_restate, pr_restate_decisions

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')


def _fixture16(seed, n_real, n_gen):
    return tuple(torch.from_numpy(x).to(torch.float16) for x in pr_fixture(seed, n_real, n_gen))


@pytest.mark.parametrize('seed,n_real,n_gen', PR_CASES)
def test_distances_match_the_restatement(seed, n_real, n_gen):
    """sidlsg_pr_distances, element by element: the restatement's fp16 value wherever the error bound e (pr_error_bound) cannot move
    the distance across an fp16 rounding boundary; elsewhere a value from fp16(d (1 - e)) to fp16(d (1 + e)) -- one of two neighbouring
    fp16 numbers, except for the few close pairs whose e exceeds an fp16 ulp (d = 5 between vectors of squared norm 1 500: e = 1e-3,
    three fp16 steps); where e reaches 1 (a row against itself) that is anything from 0 to fp16(2 d).  The share of boundary elements is
    computed on the CPU and capped at 10 %."""
    _need_gpu()
    from sid_lsg_amd import ops
    real, gen = _fixture16(seed, n_real, n_gen)
    for rows, cols in ((gen, real), (real, real), (real, gen), (gen, gen)):
        r = pr_restate(rows, cols)
        out = ops.pr_distances(rows.cuda(), cols.cuda()).cpu()
        assert out.dtype == torch.float16 and out.shape == r['exact'].shape
        boundary = r['lo'] != r['hi']
        share = float(boundary.float().mean())
        exact_ok = out == r['exact']
        within = (out >= r['lo']) & (out <= r['hi'])
        print(f'seed {seed} {tuple(out.shape)}: boundary share {share:.4f}, differ from fp16(d) on {float((~exact_ok).float().mean()):.5f}, '
              f'wide {int(r["wide"].sum())}')
        assert share <= 0.10
        assert bool(torch.where(boundary, within, exact_ok).all())


def _sets():
    real1, _ = _fixture16(1, 416, 352)
    real2, _ = _fixture16(2, 1216, 1088)
    dup = torch.cat([real1[:300], real1[:10].repeat(5, 1), real1[20:23]])[torch.randperm(353, generator=torch.Generator().manual_seed(0))]
    return dict(n416=real1, n1216=real2, duplicates=dup)


@pytest.mark.parametrize('k', [1, 3, 7])
def test_kth_radius_is_kthvalue_of_the_dense_matrix(k):
    """The fused radius = kthvalue(k + 1) of the kernel's OWN dense matrix, bit for bit (same arithmetic on both paths): N = 416 and
    1 216, a set with duplicated rows (ties, radius 0) and one with N = k + 1."""
    _need_gpu()
    from sid_lsg_amd import ops
    sets = _sets()
    sets['n_is_k_plus_1'] = sets['n1216'][:k + 1]
    for name, feats in sets.items():
        m = feats.cuda()
        dense = ops.pr_distances(m, m)
        want = kth(dense, k)
        got = ops.pr_kth_radius(m, k)
        assert got.dtype == torch.float16 and torch.equal(got, want), (name, k, int((got != want).sum()))
        assert bool((dense.diagonal() == 0).all()) and bool((dense.float().min(1).values == 0).all())     # self: exactly 0, the smallest
    if k == 3:
        assert int((ops.pr_kth_radius(sets['duplicates'].cuda(), 3) == 0).sum()) >= 60       # the rows that occur 6 times
    # k > 7: the dense fallback, same distances
    m = sets['n416'].cuda()
    assert torch.equal(ops.pr_kth_radius(m, 9), kth(ops.pr_distances(m, m), 9))
    with pytest.raises(RuntimeError):
        ops.pr_kth_radius(m[:3], 3)


@pytest.mark.parametrize('seed,n_real,n_gen', PR_CASES)
def test_member_matches_dense_and_restatement(seed, n_real, n_gen):
    """sidlsg_pr_member = (dense <= radius).any(1) of the kernel's own dense matrix, bit for bit; and the restatement's decision on
    every robust probe.  Fragile probes: at most 0.5 % of a probe set."""
    _need_gpu()
    from sid_lsg_amd import ops
    real, gen = _fixture16(seed, n_real, n_gen)
    for name, manifold, probes in (('precision', real, gen), ('recall', gen, real)):
        m, p = manifold.cuda(), probes.cuda()
        radius = ops.pr_kth_radius(m, PR_K)
        got = ops.pr_member(p, m, radius)
        assert got.dtype == torch.bool and torch.equal(got, (ops.pr_distances(p, m) <= radius).any(1))
        inside, robust, _ = pr_restate_decisions(manifold, probes, PR_K)
        fragile = int((~robust).sum())
        print(f'seed {seed} {name}: {fragile} fragile of {len(probes)}, kernel != restatement on {int((got.cpu() != inside).sum())}')
        assert fragile <= 0.005 * len(probes)
        assert torch.equal(got.cpu()[robust], inside[robust])
    # a radius of its own: nobody is inside a manifold of radius 0 but the manifold's own rows
    zero = torch.zeros(n_real, dtype=torch.float16, device='cuda')
    assert not bool(ops.pr_member(gen.cuda(), real.cuda(), zero).any()) and bool(ops.pr_member(real.cuda(), real.cuda(), zero).all())


def test_feature_width_is_padded_and_arguments_are_checked():
    _need_gpu()
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    real, gen = _fixture16(1, 416, 352)
    a, b = real[:130, :1000].contiguous().cuda(), gen[:70, :1000].contiguous().cuda()      # F = 1000 -> padded to 1024
    r = pr_restate(a.cpu(), b.cpu())
    out = ops.pr_distances(a, b).cpu()
    assert bool(((out >= r['lo']) & (out <= r['hi'])).all())
    with pytest.raises(RuntimeError):
        ops.pr_distances(a.float(), b)
    x = torch.zeros(64, 48, dtype=torch.float16, device='cuda')
    o = torch.zeros(64, 64, dtype=torch.float16, device='cuda')
    assert lib.sidlsg_pr_distances.raw(x.data_ptr(), 64, x.data_ptr(), 64, 48, o.data_ptr(), None) != 0           # F % 32
    assert lib.sidlsg_pr_kth_radius.raw(x.data_ptr(), 64, 32, 8, o.data_ptr(), None) != 0                          # k > 7
    assert lib.sidlsg_pr_kth_radius.raw(x.data_ptr(), 3, 32, 3, o.data_ptr(), None) != 0                           # N < k + 1
    assert lib.sidlsg_pr_member.raw(x.data_ptr(), 64, x.data_ptr(), 64, 32, None, o.data_ptr(), None) != 0         # no radius


class _Features:
    def __init__(self, x):
        self.x = x

    def get_all_torch(self):
        return self.x


@pytest.mark.parametrize('seed,n_real,n_gen', PR_CASES)
def test_compute_pr_matches_the_recorded_reference(seed, n_real, n_gen, golden_dir, monkeypatch):
    """metrics.compute_pr on the fixture's features: |precision - reference| and |recall - reference| <= (fragile probes + probes on
    which the recorded reference differs from the restatement) / n; both counts from pr_ref.npz and the CPU restatement."""
    _need_gpu()
    from sid_lsg_amd import metrics
    g = np.load(os.path.join(golden_dir, 'pr_ref.npz'))
    real32, gen32 = (torch.from_numpy(x) for x in pr_fixture(seed, n_real, n_gen))
    monkeypatch.setattr(metrics, 'dataset_feature_stats', lambda opts, max_items=None, capture_all=False: _Features(real32.cuda()[:max_items]))
    monkeypatch.setattr(metrics, 'generator_feature_stats',
                        lambda opts, num_gen, compute_clip=False, capture_all=False: (_Features(gen32.cuda()[:num_gen]), float('nan'), float('nan')))
    opts = metrics.MetricOptions(G=None, prompts=['unused'], device='cuda')
    precision, recall = metrics.compute_pr(opts, max_real=None, num_gen=n_gen, nhood_size=PR_K)
    tag = f'{seed}_{n_real}_{n_gen}'
    real, gen = real32.to(torch.float16), gen32.to(torch.float16)
    for name, value, manifold, probes in (('precision', precision, real, gen), ('recall', recall, gen, real)):
        inside, robust, _ = pr_restate_decisions(manifold, probes, PR_K)
        differ = int((torch.from_numpy(g[f'{name}_inside_{tag}']) != inside).sum())
        allowed = (int((~robust).sum()) + differ) / len(probes)
        print(f'{tag} {name}: {value:.6f}, reference {float(g[f"{name}_{tag}"]):.6f}, allowed {allowed:.6f}')
        # the recorded number is the reference's fp32 mean of the decisions: count / n rounded to fp32, i.e. off by up to 2^-24
        assert abs(value - float(g[f'{name}_{tag}'])) <= allowed + 2.0 ** -24


# ------------------------------------------------------------------------------------------------
def _image_folder(root, n=9, size=512):
    import PIL.Image
    rs = np.random.RandomState(11)
    os.makedirs(root)
    first = None
    for i in range(n):
        arr = rs.randint(0, 256, (size, size, 3)).astype(np.uint8)
        if i == 4:
            arr = arr[..., 0]               # one grey image
        first = arr if i == 0 else first
        PIL.Image.fromarray(arr).save(os.path.join(root, f'img_{i:03d}.png'))
        with open(os.path.join(root, f'img_{i:03d}.txt'), 'wt') as f:
            f.write(f'evaluation caption {i}\n')
    return first


def test_cli_fid_and_pr_from_an_image_folder(tmp_path):
    """sid_train.py --metrics fid_test,pr_test --snapshot_images 1 on random:tiny with an image folder as --data and WITHOUT
    --data_stat: the real-set statistics come from the images (cached as real_stats.npz), precision / recall from the kernels,
    reals.png shows the folder's first images.  The same with --train_mode 0."""
    _need_gpu()
    import PIL.Image
    from click.testing import CliRunner
    import sid_train
    from sid_lsg_amd import metrics

    class Detector(torch.nn.Module):        # the stand-in of tests/test_gpu_cli.py::test_train_with_fid_metric
        def __init__(self):
            super().__init__()
            torch.manual_seed(0)
            self.conv = torch.nn.Conv2d(3, 16, 8, stride=8)

        def forward(self, img: torch.Tensor, return_features: bool = True) -> torch.Tensor:
            return self.conv(img.to(torch.float32) / 255.0).mean(dim=(2, 3))
    det_path = str(tmp_path / 'detector.pt')
    torch.jit.script(Detector()).save(det_path)
    (tmp_path / 'aesthetics_6_plus.txt').write_text('\n'.join(f'prompt number {i}' for i in range(40)) + '\n')
    data = str(tmp_path / 'coco')
    first = _image_folder(data)
    runs = tmp_path / 'runs'
    common = ['--outdir', str(runs), '--data_prompt_text', str(tmp_path), '--data', data, '--sd_model', 'random:tiny', '--seed', '1',
              '--resolution', '512', '--metrics', 'fid_test,pr_test', '--metric_pt_path', det_path, '--snapshot_images', '1']
    res = CliRunner().invoke(sid_train.main, common + ['--batch', '4', '--batch-gpu', '2', '--duration', '0.00002', '--ema', '0.00001',
                                                       '--tick', '1', '--snap', '1', '--dump', '50'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    run_dir = glob.glob(str(runs / '00000-*'))[0]

    def check(directory):
        stat = os.path.join(directory, 'real_stats.npz')
        assert os.path.isfile(stat)
        mu, sigma = metrics.load_real_stats(stat)
        assert mu.shape == (16,) and sigma.shape == (16, 16) and np.isfinite(mu).all() and np.isfinite(sigma).all()
        reals = np.asarray(PIL.Image.open(os.path.join(directory, 'reals.png')).convert('RGB'))
        assert reals.shape == (4 * 512, 7 * 512, 3)             # the 7 x 4 grid of 512 x 512 tiles
        assert (reals[:512, :512] == first).all()
    check(run_dir)
    pr_files = glob.glob(os.path.join(run_dir, 'metric-pr_test*.jsonl'))
    assert pr_files, os.listdir(run_dir)
    rows = [json.loads(ln) for ln in open(pr_files[0])]
    assert rows
    for r in rows:
        vals = [r['results']['pr30k3_full_precision'], r['results']['pr30k3_full_recall']]
        assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in vals), vals
    fid = [json.loads(ln) for ln in open(glob.glob(os.path.join(run_dir, 'metric-fid_test-alpha-*.jsonl'))[0])]
    assert fid and all(np.isfinite(r['results']['fid30k_full']) for r in fid)
    assert os.path.isfile(os.path.join(run_dir, 'fakes_init.png'))
    opts_json = json.load(open(os.path.join(run_dir, 'training_options.json')))
    assert opts_json['dataset_kwargs']['class_name'] == 'sid_lsg_amd.data.ImageCaptionDataset' and opts_json['metric_real_stats'] is None

    snaps = sorted(glob.glob(os.path.join(run_dir, 'network-snapshot-*.pkl')))
    assert snaps
    ev = CliRunner().invoke(sid_train.main, common + ['--train_mode', '0', '--network_pkl', snaps[-1]], catch_exceptions=False)
    assert ev.exit_code == 0, ev.output
    ev_dir = glob.glob(str(runs / '00001-*'))[0]
    kimg = snaps[-1][-10:-4]
    for steps in (1, 2, 4):
        body = open(os.path.join(str(runs), f'pr_test{kimg}_{steps}.txt')).read()
        assert 'metric: pr_test' in body      # the evaluation branch writes the reference's `key: value` files, not jsonl lines
        vals = [float(v) for v in __import__('re').findall(r"'pr30k3_full_(?:precision|recall)': ([0-9.e+-]+)", body)]
        assert len(vals) == 2 and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in vals), body
    check(ev_dir)
    # neither --data_stat nor images: the error of before, word for word
    bad = CliRunner().invoke(sid_train.main, ['--outdir', str(runs), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny',
                                              '--metrics', 'fid_test', '--metric_pt_path', det_path, '-n'])
    assert bad.exit_code != 0 and "--metrics needs --data_stat to be a local file (got None)" in bad.output
    bad = CliRunner().invoke(sid_train.main, ['--outdir', str(runs), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny',
                                              '--metrics', 'pr_test', '--metric_pt_path', det_path, '--data_stat', det_path, '-n'])
    assert bad.exit_code != 0 and '--data' in bad.output
