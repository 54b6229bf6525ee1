"""KID and CMMD without a GPU: the subset draw, the arithmetic around the kernel sums against the literal published formulas in fp64
numpy (explicit m x m matrices), the registry and the command-line checks.  The restatements here are also the reference of
tests/test_gpu_kernel_metrics.py."""
import json
import os

import numpy as np
import pytest

POLY3, RBF = 0, 1


# ---- the fp64 restatement ------------------------------------------------------------------------------------------------
def restate_kernel_matrix(a, b, kind, p0, p1=0.0):
    """[len(a), len(b)] fp64: what sidlsg_pair_kernel_sums sums -- (p0 a.b + p1)^3, or 1 - exp(-p0 |a - b|^2) with the squared
    distance formed from the differences themselves (no cancellation of norms)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if kind == POLY3:
        return (p0 * (a @ b.T) + p1) ** 3
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return -np.expm1(-p0 * d2)


def restate_sums(x, y, kind, p0, p1=0.0):
    """(Sxx, Syy, Sxy, Txx, Tyy) in fp64."""
    kxx, kyy, kxy = (restate_kernel_matrix(a, b, kind, p0, p1) for a, b in ((x, x), (y, y), (x, y)))
    return np.array([kxx.sum(), kyy.sum(), kxy.sum(), np.trace(kxx), np.trace(kyy)])


def restate_kid(gen, real, ix, iy):
    """StyleGAN3 metrics/kernel_inception_distance.py, line for line, on given subsets (n = the feature width)."""
    gen, real = np.asarray(gen, np.float64), np.asarray(real, np.float64)
    n, m, t = real.shape[1], ix.shape[1], 0.0
    for sx, sy in zip(ix, iy):
        x, y = gen[sx], real[sy]
        a = (x @ x.T / n + 1) ** 3 + (y @ y.T / n + 1) ** 3
        b = (x @ y.T / n + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (m - 1) - b.sum() * 2 / m
    return t / len(ix) / m


def restate_cmmd(x, y, sigma=10.0, scale=1000.0):
    """The published CMMD `mmd(x, y)` (distance.py), in fp64: RBF kernel means with the diagonal, gamma = 1 / (2 sigma^2)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    gamma = 1.0 / (2.0 * sigma ** 2)
    xs, ys = (x * x).sum(1), (y * y).sum(1)
    k_xx = np.mean(np.exp(-gamma * (-2.0 * x @ x.T + xs[:, None] + xs[None, :])))
    k_xy = np.mean(np.exp(-gamma * (-2.0 * x @ y.T + xs[:, None] + ys[None, :])))
    k_yy = np.mean(np.exp(-gamma * (-2.0 * y @ y.T + ys[:, None] + ys[None, :])))
    return scale * (k_xx + k_yy - 2.0 * k_xy)


def unit_rows(rs, n, F, shift=0.0):
    x = rs.randn(n, F) + shift
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ---- kid_subsets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_gen,n_real,cap,m', [(50, 70, 1000, 50), (70, 50, 1000, 50), (70, 90, 40, 40)])
def test_kid_subsets(n_gen, n_real, cap, m):
    from sid_lsg_amd import metrics
    ix, iy = metrics.kid_subsets(n_gen, n_real, 7, cap, seed=3)
    assert ix.shape == iy.shape == (7, m) and ix.dtype == iy.dtype == np.int32
    for rows, n in ((ix, n_gen), (iy, n_real)):
        assert rows.min() >= 0 and rows.max() < n
        assert all(len(set(r.tolist())) == m for r in rows), 'drawn without replacement'
    again = metrics.kid_subsets(n_gen, n_real, 7, cap, seed=3)
    assert (again[0] == ix).all() and (again[1] == iy).all()
    other = metrics.kid_subsets(n_gen, n_real, 7, cap, seed=4)
    assert not ((other[0] == ix).all() and (other[1] == iy).all())
    # the draw order of kernel_inception_distance.py: per subset the generated rows first, then the real ones
    rnd = np.random.RandomState(3)
    assert (rnd.choice(n_gen, m, replace=False) == ix[0]).all() and (rnd.choice(n_real, m, replace=False) == iy[0]).all()


# ---- the arithmetic around the sums ----------------------------------------------------------------------------------------
def test_kid_from_sums_is_the_published_estimator():
    from sid_lsg_amd import metrics
    rs = np.random.RandomState(0)
    F = 24
    gen, real = (rs.randn(90, F) * 1.5 + 0.3).astype(np.float32), rs.randn(120, F).astype(np.float32)
    ix, iy = metrics.kid_subsets(len(gen), len(real), 5, 40, seed=1)
    sums = np.stack([restate_sums(gen[sx], real[sy], POLY3, 1.0 / F, 1.0) for sx, sy in zip(ix, iy)])
    want = restate_kid(gen, real, ix, iy)
    got = metrics.kid_from_sums(sums, 40)
    print(f'KID {got:.15e}, restatement {want:.15e}')
    assert want > 0 and abs(got - want) <= 1e-12 * abs(want)
    assert np.isnan(metrics.kid_from_sums(sums, 1))        # no pair i != j: the 0 / 0 of the published code


def test_cmmd_from_sums_is_the_published_estimator():
    from sid_lsg_amd import metrics
    rs = np.random.RandomState(1)
    x, y = unit_rows(rs, 60, 32, shift=0.0), unit_rows(rs, 75, 32, shift=0.6)
    gamma = 1.0 / (2.0 * metrics.CMMD_SIGMA ** 2)
    want = restate_cmmd(x, y)
    got = metrics.cmmd_from_sums(restate_sums(x, y, RBF, gamma), len(x), len(y))
    print(f'CMMD {got:.15e}, restatement {want:.15e}')
    assert want > 0.1 and abs(got - want) <= 1e-12 * abs(want)
    # a set against itself: the three sums are the same number and cancel
    same = metrics.cmmd_from_sums(restate_sums(x, x, RBF, gamma), len(x), len(x))
    assert abs(same) <= 1e-12


def test_kid_of_two_halves_of_one_sample_is_zero_within_its_standard_error():
    from sid_lsg_amd import metrics
    rs = np.random.RandomState(2)
    F, m, S = 16, 50, 40
    pool = rs.randn(4000, F).astype(np.float32)
    a, b = pool[:2000], pool[2000:]
    ix, iy = metrics.kid_subsets(len(a), len(b), S, m, seed=0)
    sums = np.stack([restate_sums(a[sx], b[sy], POLY3, 1.0 / F, 1.0) for sx, sy in zip(ix, iy)])
    per_subset = (((sums[:, 0] - sums[:, 3]) + (sums[:, 1] - sums[:, 4])) / (m - 1) - 2.0 * sums[:, 2] / m) / m
    kid = metrics.kid_from_sums(sums, m)
    stderr = per_subset.std(ddof=1) / np.sqrt(S)
    print(f'KID {kid:.3e}, standard error over the subsets {stderr:.3e}')
    assert abs(kid - per_subset.mean()) <= 1e-15 and abs(kid) <= 3.0 * stderr


# ---- registry and options --------------------------------------------------------------------------------------------------
def test_metrics_are_registered_behind_the_existing_ones():
    from sid_lsg_amd import clip, metrics
    names = metrics.list_valid_metrics()
    assert names[:4] == ['fid30k_full', 'fid_clip_30k_full', 'fid_test', 'fid_clip_test']
    assert names[-4:] == ['kid30k_full', 'kid_test', 'cmmd30k_full', 'cmmd_test']
    assert all(metrics.is_valid_metric(n) for n in names[-4:])
    assert metrics.HPS_METRICS == ('hpsv2', 'hpsv2_test')
    assert set(names[-4:]) <= set(metrics.NEEDS_IMAGES) and set(metrics.CMMD_METRICS) == {'cmmd30k_full', 'cmmd_test'}
    v, _ = clip.parse_clip_config(clip.CLIP_ARCHS['vit-l-14-336'])
    assert (v.image_size, v.patch_size, v.hidden_size) == (336, 14, 1024)


def _image_folder(root, n=3):
    import PIL.Image
    rs = np.random.RandomState(5)
    os.makedirs(root)
    for i in range(n):
        PIL.Image.fromarray(rs.randint(0, 256, (8, 8, 3)).astype(np.uint8)).save(os.path.join(root, f'img_{i}.png'))
        with open(os.path.join(root, f'img_{i}.txt'), 'wt') as f:
            f.write(f'caption {i}\n')
    return root


def test_command_line_checks(tmp_path):
    from click.testing import CliRunner
    import sid_train
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a red cube\na blue sphere\n')
    images = _image_folder(str(tmp_path / 'coco'))
    captions = tmp_path / 'captions.txt'
    captions.write_text('one\ntwo\n')
    det = tmp_path / 'detector.pt'
    det.write_bytes(b'stand-in')
    base = ['--outdir', str(tmp_path / 'runs'), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny', '--seed', '1', '--dry-run']
    run =lambda *extra: CliRunner().invoke(sid_train.main, base + list(extra))      # noqa: E731
    bad = run('--metrics', 'cmmd_test', '--data', images)
    assert bad.exit_code != 0 and '--metric_cmmd_clip_path' in bad.output, bad.output
    # cmmd alone: neither --metric_pt_path nor --data_stat
    ok = run('--metrics', 'cmmd_test', '--data', images, '--metric_cmmd_clip_path', 'random:clip-tiny')
    assert ok.exit_code == 0, ok.output
    opts = json.loads(ok.output[ok.output.index('{'):ok.output.rindex('}') + 1])
    assert opts['metric_cmmd_clip_path'] == 'random:clip-tiny' and opts['metric_pt_path'] is None and opts['metric_real_stats'] is None
    assert opts['dataset_kwargs']['class_name'] == 'sid_lsg_amd.data.ImageCaptionDataset'
    # kid needs the Inception file, and the images themselves
    bad = run('--metrics', 'kid_test', '--data', images)
    assert bad.exit_code != 0 and '--metrics needs --metric_pt_path to be a local file' in bad.output, bad.output
    ok = run('--metrics', 'kid_test', '--data', images, '--metric_pt_path', str(det))
    assert ok.exit_code == 0, ok.output
    bad = run('--metrics', 'kid_test', '--data', str(captions), '--metric_pt_path', str(det))
    assert bad.exit_code != 0 and 'read the real images' in bad.output, bad.output


def test_options_reach_every_evaluation_entry():
    import inspect
    from sid_lsg_amd import metrics
    from sid_lsg_amd.training_loop import evaluate_network, evaluate_teacher, training_loop
    for fn in (training_loop, evaluate_network, evaluate_teacher, metrics.MetricOptions.__init__):
        assert inspect.signature(fn).parameters['metric_cmmd_clip_path'].default is None


def test_dry_run_without_the_option_prints_what_it_printed(tmp_path, golden_dir, monkeypatch):
    from click.testing import CliRunner
    import sid_train
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a red cube\na blue sphere\n')
    monkeypatch.chdir(tmp_path)
    res = CliRunner().invoke(sid_train.main, [
        '--outdir', 'runs', '--data_prompt_text', '.', '--sd_model', 'random:tiny', '--seed', '3', '--batch', '8', '--batch-gpu', '2',
        '--duration', '0.01', '--ema', '0.05', '--cfg_train_fake', '1.5', '--cfg_eval_fake', '1.5', '--cfg_eval_real', '1.5', '--dry-run'])
    assert res.exit_code == 0, res.output
    with open(os.path.join(golden_dir, 'sid_train_dry_run.txt')) as f:
        assert res.output == f.read()
    assert 'metric_cmmd_clip_path' not in res.output
