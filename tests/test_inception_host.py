"""Host side of the Inception-v3 detector (sid_lsg_amd/inception.py) and of the Inception Score (metrics.compute_is): the state-dict
loader, the BatchNorm folding, the integer resize plan, the IS arithmetic and the registry.  No GPU."""
import numpy as np
import pytest
import torch

import inception_ref as R


@pytest.fixture(scope='module')
def seeded_sd():
    return R.seeded_net(0).state_dict()


def restate_is(p, num_splits):
    """exp(mean_i KL(p_i || mean_i p_i)) per contiguous split, in numpy fp64 -> (mean, population std)."""
    p = np.asarray(p, dtype=np.float64)
    n = p.shape[0]
    scores = []
    for s in range(num_splits):
        q = p[s * n // num_splits:(s + 1) * n // num_splits]
        m = q.mean(0)
        kl = 0.0
        for row in q:
            nz = row > 0
            kl += float((row[nz] * (np.log(row[nz]) - np.log(m[nz]))).sum())
        scores.append(np.exp(kl / len(q)))
    return float(np.mean(scores)), float(np.std(scores))


# ---- loader -------------------------------------------------------------------------------------------------------------------
def test_conv_table_is_the_network():
    from sid_lsg_amd import inception
    table, widths = inception.conv_table()
    assert len(table) == 94 and widths['Mixed_5b'] == 192 and widths['Mixed_6a'] == 288 and widths['Mixed_7a'] == 768 and widths['Mixed_7c'] == 2048
    shapes = inception.expected_shapes()
    ref = {k: tuple(v.shape) for k, v in R.InceptionV3Ref().state_dict().items() if not k.endswith('num_batches_tracked')}
    assert shapes == ref
    assert sum(int(np.prod(s)) for s in shapes.values()) == 23885392


def test_state_dict_round_trips_through_torch_save(tmp_path, seeded_sd):
    from sid_lsg_amd import inception
    for name, obj in (('plain.pth', seeded_sd), ('wrapped.pth', {'state_dict': seeded_sd, 'epoch': 3})):
        path = str(tmp_path / name)
        torch.save(obj, path)
        sd = inception.load_state_dict_file(path)
        assert sd is not None
        got = inception.check_state_dict(sd)
        assert set(got) == set(inception.expected_shapes())
        assert all(torch.equal(got[k], seeded_sd[k]) for k in got)
    assert not any(k.endswith('num_batches_tracked') for k in got)


def test_loader_refuses_by_name(seeded_sd):
    from sid_lsg_amd import inception
    sd = dict(seeded_sd)
    del sd['Mixed_6c.branch7x7dbl_3.bn.running_var']
    with pytest.raises(KeyError, match='Mixed_6c.branch7x7dbl_3.bn.running_var'):
        inception.check_state_dict(sd)
    sd = dict(seeded_sd)
    sd['fc.weight'] = torch.zeros(1000, 2048)
    with pytest.raises(ValueError, match=r"'fc.weight' has shape \(1000, 2048\), expected \(1008, 2048\)"):
        inception.check_state_dict(sd)
    sd = dict(seeded_sd)
    sd['Mixed_7a.branch7x7x3_2.conv.weight'] = sd['Mixed_7a.branch7x7x3_2.conv.weight'].transpose(2, 3)
    with pytest.raises(ValueError, match='Mixed_7a.branch7x7x3_2.conv.weight'):
        inception.check_state_dict(sd)


def test_loader_ignores_aux_logits(seeded_sd):
    from sid_lsg_amd import inception
    sd = dict(seeded_sd)
    sd['AuxLogits.conv0.conv.weight'] = torch.zeros(128, 768, 1, 1)
    sd['AuxLogits.fc.weight'] = torch.zeros(7, 7)          # not even a sensible shape: never looked at
    got = inception.check_state_dict(sd)
    assert not any(k.startswith('AuxLogits') for k in got) and len(got) == len(inception.expected_shapes())


def test_files_that_are_not_state_dicts_are_left_to_the_old_chain(tmp_path):
    from sid_lsg_amd import inception

    class Detector(torch.nn.Module):
        def forward(self, img: torch.Tensor, return_features: bool = True) -> torch.Tensor:
            return img.to(torch.float32).mean(dim=(2, 3))
    script = str(tmp_path / 'detector.pt')
    torch.jit.script(Detector()).save(script)
    assert inception.load_state_dict_file(script) is None
    other = str(tmp_path / 'other.pth')
    torch.save({'mu': torch.zeros(3)}, other)
    assert inception.load_state_dict_file(other) is None
    assert inception.is_random_spec('random:inception-v3') and inception.is_random_spec('random:inception-v3:7')
    assert not inception.is_random_spec('random:inception-v4') and not inception.is_random_spec(None)


def test_random_state_dict_is_seeded_and_complete():
    from sid_lsg_amd import inception
    a, b, c = inception.random_state_dict(0), inception.random_state_dict(0), inception.random_state_dict(1)
    assert set(a) == set(inception.expected_shapes())
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a['fc.weight'], c['fc.weight'])
    inception.check_state_dict(a)
    w = a['Mixed_5b.branch5x5_2.conv.weight']
    assert abs(float(w.std()) - (2.0 / (48 * 25)) ** 0.5) < 0.02 * (2.0 / (48 * 25)) ** 0.5
    v = a['Mixed_5b.branch5x5_2.bn.running_var']
    assert 0.5 <= float(v.min()) and float(v.max()) <= 1.5


# ---- BatchNorm folding --------------------------------------------------------------------------------------------------------
def test_bn_fold_is_the_fp64_formula_rounded_once(seeded_sd):
    from sid_lsg_amd import inception
    for key in ('Conv2d_1a_3x3', 'Mixed_6b.branch7x7_2', 'Mixed_7c.branch3x3dbl_3b'):
        w, g, b, m, v = (seeded_sd[f'{key}.{n}'] for n in ('conv.weight', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var'))
        fw, fb = inception.fold_bn(w, g, b, m, v)
        w64, g64, b64, m64, v64 = (t.numpy().astype(np.float64) for t in (w, g, b, m, v))
        s = g64 / np.sqrt(v64 + 1e-3)
        assert fw.dtype == torch.float32 and fb.dtype == torch.float32
        assert np.array_equal(fw.numpy(), (w64 * s[:, None, None, None]).astype(np.float32))
        assert np.array_equal(fb.numpy(), (b64 - m64 * s).astype(np.float32))


def test_folded_conv_equals_conv_bn(seeded_sd):
    """The folding is the right algebra: conv + eval BatchNorm in fp64 against the folded convolution in fp64."""
    from sid_lsg_amd import inception
    key = 'Mixed_5b.branch5x5_2'
    w, g, b, m, v = (seeded_sd[f'{key}.{n}'] for n in ('conv.weight', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var'))
    x = torch.randn(2, 48, 6, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, w.double(), padding=2), m.double(), v.double(), g.double(), b.double(), False, 0.0, 1e-3)
    fw, fb = inception.fold_bn(w, g, b, m, v)
    got = torch.nn.functional.conv2d(x, fw.double(), fb.double(), padding=2)
    assert float((got - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())


# ---- resize plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [256, 64, 48, 512, 299])
def test_resize_plan_is_the_integer_form_of_the_legacy_tf_rule(size):
    from fractions import Fraction
    from sid_lsg_amd import inception
    q, rem, q1 = inception.resize_plan(size)
    assert q.shape == rem.shape == q1.shape == (299,)
    for i in range(299):
        pos = Fraction(i * size, 299)
        assert q[i] == pos.numerator // pos.denominator and Fraction(int(rem[i]), 299) == pos - int(q[i])
        assert q1[i] == min(q[i] + 1, size - 1)
    assert 0 <= rem.min() and rem.max() < 299 and q.max() <= size - 1
    if size == 299:
        assert np.array_equal(q, np.arange(299)) and not rem.any()
    # the last tap clamps to the border exactly where the +1 neighbour would leave the image
    assert q1[-1] == size - 1 and np.array_equal(q1 == q, q == size - 1)


def test_resize_plan_reproduces_the_grid_sample_form():
    """The plan, evaluated in fp64, against the affine_grid / grid_sample pair in fp64 (the resize inside the TorchScript detector)."""
    from sid_lsg_amd import inception
    img = R.structured_images(1, 64, 48, seed=3)
    want = R.resize_299(img.double())
    x = img.double()
    q, rem, q1 = inception.resize_plan(48)
    lx = torch.from_numpy(rem / 299.0)
    rows = x[..., q] + lx * (x[..., q1] - x[..., q])
    q, rem, q1 = inception.resize_plan(64)
    ly = torch.from_numpy(rem / 299.0)[:, None]
    got = rows[..., q, :] + ly * (rows[..., q1, :] - rows[..., q, :])
    assert float((got - want).abs().max()) <= 1e-10
    assert float((R.legacy_tf_resize_299(img) - want).abs().max()) <= 1e-10


# ---- Inception Score ----------------------------------------------------------------------------------------------------------
def test_is_matches_the_numpy_restatement():
    from sid_lsg_amd import metrics
    rs = np.random.RandomState(5)
    logits = rs.normal(0, 2.0, (53, 17))
    p = np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
    p[3, :5] = 0.0                                  # exact zeros: 0 log 0 = 0
    p[3] /= p[3].sum()
    for splits in (1, 4, 10):
        got, want = metrics.is_from_probabilities(p, splits), restate_is(p, splits)
        assert abs(got[0] - want[0]) <= 1e-12 * want[0] and abs(got[1] - want[1]) <= 1e-12 * want[0]
    assert metrics.is_from_probabilities(p, 10)[1] > 0
    with pytest.raises(ValueError):
        metrics.is_from_probabilities(p[:3], 10)


def test_is_of_one_hot_and_uniform_rows():
    from sid_lsg_amd import metrics
    K, C = 8, 1008
    onehot = np.zeros((5 * K, C))
    onehot[np.arange(5 * K), np.arange(5 * K) % K] = 1.0         # every one of K classes 5 times
    mean, std = metrics.is_from_probabilities(onehot, 1)
    assert mean == K and std == 0.0
    mean, std = metrics.is_from_probabilities(np.tile(onehot[:K], (10, 1)), 10)        # each split holds the K classes once
    assert mean == K and std == 0.0
    mean, std = metrics.is_from_probabilities(np.full((40, C), 1.0 / C), 10)
    assert mean == 1.0 and std == 0.0


# ---- registry and interface ---------------------------------------------------------------------------------------------------
def test_is_metrics_are_registered():
    from sid_lsg_amd import metrics
    assert metrics.is_valid_metric('is30k_full') and metrics.is_valid_metric('is_test')
    assert metrics.IS_METRICS == ('is30k_full', 'is_test')
    assert not set(metrics.IS_METRICS) & set(metrics.NEEDS_IMAGES)
    assert metrics.is_inception_spec('random:inception-v3') and metrics.is_inception_spec('random:inception-v3:3')
    assert not metrics.is_inception_spec('random:clip-tiny') and not metrics.is_clip_spec('random:inception-v3')


def test_load_detector_takes_a_state_dict_file(tmp_path, seeded_sd, monkeypatch):
    """A torch.save'd state dict reaches HipInceptionV3 (until now it ended in pickle.load failing).  No GPU here: the class is
    replaced by a recorder of what load_detector hands it."""
    from sid_lsg_amd import inception, metrics
    seen = {}

    class Recorder:
        def __init__(self, sd, device, **kw):
            seen['sd'], seen['device'] = inception.check_state_dict(sd), device
    monkeypatch.setattr(inception, 'HipInceptionV3', Recorder)
    path = str(tmp_path / 'pt_inception.pth')
    torch.save(seeded_sd, path)
    det = metrics.load_detector(path, 'cpu')
    assert isinstance(det, Recorder) and seen['device'] == 'cpu' and torch.equal(seen['sd']['fc.bias'], seeded_sd['fc.bias'])
    det = metrics.load_detector('random:inception-v3:4', 'cpu')
    assert isinstance(det, Recorder) and torch.equal(seen['sd']['fc.bias'], inception.random_state_dict(4)['fc.bias'])
    # a broken state dict is refused by name, not handed on to torch.jit / pickle
    bad = dict(seeded_sd)
    del bad['fc.bias']
    torch.save(bad, path)
    with pytest.raises(KeyError, match='fc.bias'):
        metrics.load_detector(path, 'cpu')


def test_cli_gating_for_the_inception_score(tmp_path):
    """is_test asks for neither --data_stat nor real images; random:inception-v3 passes for --metric_pt_path; a missing file does not."""
    from click.testing import CliRunner
    import sid_train
    (tmp_path / 'aesthetics_6_plus.txt').write_text('\n'.join(f'prompt {i}' for i in range(20)) + '\n')

    def run(*extra):
        return CliRunner().invoke(sid_train.main, ['--outdir', str(tmp_path / 'runs'), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny',
                                                   '--seed', '1', '--dry-run', *extra])
    ok = run('--metrics', 'is_test', '--metric_pt_path', 'random:inception-v3')
    assert ok.exit_code == 0, ok.output
    bad = run('--metrics', 'is_test')
    assert bad.exit_code != 0 and '--metrics needs --metric_pt_path to be a local file' in bad.output, bad.output
    bad = run('--metrics', 'is_test,fid_test', '--metric_pt_path', 'random:inception-v3')       # fid_test still needs its statistics
    assert bad.exit_code != 0 and '--data_stat' in bad.output, bad.output
