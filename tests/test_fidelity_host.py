"""Paired fidelity without a GPU: the fp64 SSIM reference against scipy's Gaussian filter and its closed forms, the set-level rules of
`aggregate`, the weight loaders' refusals by name, and every usage error of the two command lines (refused before a GPU is touched)."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import fidelity_ref as ref
from sid_lsg_amd import fidelity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('image_pair_fidelity', os.path.join(ROOT, 'tools', 'image_pair_fidelity.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('H,W', [(11, 11), (12, 45), (43, 37)])
def test_valid_window_form_equals_the_scipy_filter(H, W):
    rng = np.random.default_rng(H * 100 + W)
    x = rng.integers(0, 256, (H, W), dtype=np.uint8)
    y = np.clip(x.astype(np.int64) + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8)
    got, want = ref.ssim_map(x, y), ref.ssim_map_scipy(x, y)
    assert got.shape == (H - 10, W - 10)
    err = np.abs(got - want).max()
    print(f'{H} x {W}: max |valid-window - scipy| = {err:.3g}')
    assert err <= 1e-12


def test_ssim_closed_forms():
    g = ref.window()
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (17, 23), dtype=np.uint8)
    assert np.all(ref.ssim_map(x, x) == 1.0)                       # exactly: numerator and denominator are the same bits
    lo, hi = np.zeros((13, 12), np.uint8), np.full((13, 12), 255, np.uint8)
    want = ref.C1 / (65025.0 + ref.C1)
    assert abs(want - 9.99900009999e-5) < 1e-15
    assert np.abs(ref.ssim_map(lo, hi) - want).max() < 1e-15
    sums = ref.psnr_ssim_sums(np.stack([lo, lo, lo])[None], np.stack([hi, hi, hi])[None])[0]
    assert sums[0] == 3 * 13 * 12 * 65025 and sums[1] == 3 * 13 * 12 and sums[3] == 3 * 3 * 2 and sums[4:6] == sums[0:2]


def test_metrics_from_sums_and_aggregate():
    rows = fidelity.metrics_from_sums([[0.0, 300.0, 100.0, 100.0, 0.0, 0.0, 0.0, 0.0],
                                       [600.0, 300.0, 50.0, 100.0, 30.0, 30.0, 9.0, 10.0]], with_keep=True)
    assert rows[0]['mse'] == 0 and rows[0]['psnr'] == math.inf and rows[0]['ssim'] == 1.0
    assert all(math.isnan(rows[0][k]) for k in fidelity.KEEP_KEYS)                 # nothing kept in image 0
    assert rows[1]['mse'] == 2.0 and rows[1]['psnr'] == pytest.approx(10 * math.log10(65025 / 2.0), rel=1e-15) and rows[1]['ssim'] == 0.5
    assert rows[1]['mse_keep'] == 1.0 and rows[1]['psnr_keep'] == pytest.approx(10 * math.log10(65025.0), rel=1e-15) and rows[1]['ssim_keep'] == 0.9
    assert sorted(fidelity.metrics_from_sums([[1.0, 1.0, 1.0, 1.0, 0, 0, 0, 0]], with_keep=False)[0]) == ['mse', 'psnr', 'ssim']
    rows[0]['lpips'], rows[1]['lpips'] = 0.0, 0.5
    mean = fidelity.aggregate(rows)
    assert sorted(mean) == sorted(fidelity.KEYS + fidelity.KEEP_KEYS + ('lpips',))
    # psnr from the MEAN mse: the identical pair does not make it infinite
    assert mean['mse'] == 1.0 and mean['psnr'] == pytest.approx(10 * math.log10(65025.0), rel=1e-15) and mean['ssim'] == 0.75 and mean['lpips'] == 0.25
    # _keep: over the images that have kept terms
    assert mean['mse_keep'] == 1.0 and mean['ssim_keep'] == 0.9 and mean['psnr_keep'] == pytest.approx(10 * math.log10(65025.0), rel=1e-15)
    assert fidelity.aggregate({'a.png': rows[0], 'b.png': rows[1]}) == mean       # a dict keyed by file name is read the same way
    same = fidelity.aggregate([rows[0]])
    assert same['psnr'] == math.inf and same['mse'] == 0 and math.isnan(same['mse_keep']) and math.isnan(same['psnr_keep']) and math.isnan(same['ssim_keep'])
    plain = fidelity.aggregate([{'mse': 4.0, 'psnr': 1.0, 'ssim': 0.25}])
    assert sorted(plain) == ['mse', 'psnr', 'ssim'] and plain['psnr'] == pytest.approx(10 * math.log10(65025 / 4.0), rel=1e-15)
    with pytest.raises(ValueError):
        fidelity.aggregate([])


def test_loader_refusals_by_name(tmp_path):
    vgg, lin = fidelity.random_state_dicts(3)
    assert len(vgg) == 26 and len(lin) == 5 and all(bool((v >= 0).all()) for v in lin.values())
    assert sorted(fidelity.check_vgg_state_dict({**vgg, 'classifier.0.weight': torch.zeros(2, 2)})) == sorted(vgg)      # classifier keys are ignored
    assert sorted(fidelity.check_vgg_state_dict({'state_dict': vgg})) == sorted(vgg)
    with pytest.raises(KeyError, match=r"features\.17\.bias"):
        fidelity.check_vgg_state_dict({k: v for k, v in vgg.items() if k != 'features.17.bias'})
    with pytest.raises(ValueError, match=r"features\.5\.weight.*\(128, 64, 3, 3\)"):
        fidelity.check_vgg_state_dict({**vgg, 'features.5.weight': torch.zeros(128, 64, 1, 1)})
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        fidelity.check_lin_state_dict({k: v for k, v in lin.items() if k != 'lin3.model.1.weight'})
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight.*\(1, 512, 1, 1\)"):
        fidelity.check_lin_state_dict({**lin, 'lin4.model.1.weight': torch.zeros(1, 256, 1, 1)})
    # a file of another network (an IP-Adapter Resampler's keys): refused by the first key this network misses, naming what the file holds
    foreign = {'latents': torch.zeros(1, 16, 8), 'proj_in.weight': torch.zeros(8, 8), 'layers.0.0.to_q.weight': torch.zeros(8, 8)}
    with pytest.raises(KeyError, match=r"features\.0\.weight.*latents"):
        fidelity.check_vgg_state_dict(foreign)
    with pytest.raises(KeyError, match=r"lin0\.model\.1\.weight.*proj_in"):
        fidelity.check_lin_state_dict(foreign)
    with pytest.raises(ValueError, match='state dict'):
        fidelity.check_vgg_state_dict([1, 2])
    # the specs: both or neither random, one seed, and files that exist -- all before a device is needed
    for bad in [('random:lpips-vgg', None), (None, 'x.pth'), ('random:lpips-vgg', 'x.pth'), ('random:lpips-vgg:1', 'random:lpips-vgg:2'),
                ('random:lpips-vgg:x', 'random:lpips-vgg:x')]:
        with pytest.raises(ValueError, match='lpips'):
            fidelity.check_specs(*bad)
    fidelity.check_specs('random:lpips-vgg:7', 'random:lpips-vgg:7')
    with pytest.raises(ValueError, match='--lpips_vgg.*not a file'):
        fidelity.load_lpips(str(tmp_path / 'none.pth'), str(tmp_path / 'lin.pth'), 'cpu')
    torch.save(foreign, tmp_path / 'foreign.pth')
    torch.save(lin, tmp_path / 'lin.pth')
    with pytest.raises(KeyError, match=r"features\.0\.weight"):
        fidelity.load_lpips(str(tmp_path / 'foreign.pth'), str(tmp_path / 'lin.pth'), 'cpu')
    # the restatement reads the same dicts through the same key names
    ref.LpipsVgg().load(vgg, lin)


def _images(d, sizes):
    import PIL.Image
    os.makedirs(d, exist_ok=True)
    for i, (w, h) in enumerate(sizes):
        PIL.Image.fromarray(np.full((h, w, 3), 10 * i, np.uint8), 'RGB').save(os.path.join(d, f'{i}.png'))
    return str(d)


def test_generate_usage_errors(tmp_path):
    from click.testing import CliRunner
    import generate_onestep as g
    init = _images(tmp_path / 'init', [(16, 16)])
    run = lambda *a: CliRunner().invoke(g.main, ['--outdir', str(tmp_path / 'o'), '--repo_id', 'random:tiny', '--network', 'x.pkl', *a])  # noqa: E731
    r = run('--fidelity', '1')
    assert r.exit_code == 2 and '--fidelity' in r.output and '--init_images' in r.output
    for opt in ('--lpips_vgg', '--lpips_lin'):
        r = run('--init_images', init, opt, 'random:lpips-vgg')
        assert r.exit_code == 2 and opt in r.output and '--fidelity' in r.output
    r = run('--init_images', init, '--fidelity', '1', '--lpips_vgg', 'random:lpips-vgg')
    assert r.exit_code == 2 and '--lpips_vgg' in r.output and '--lpips_lin' in r.output
    r = run('--init_images', init, '--fidelity', '1', '--lpips_vgg', 'random:lpips-vgg', '--lpips_lin', 'lin.pth')
    assert r.exit_code == 2 and 'for both' in r.output
    assert g.fidelity_options(None, False, None, None) is None
    assert g.fidelity_options(init, True, None, None) == (None, None)
    assert g.fidelity_options(init, True, 'random:lpips-vgg:2', 'random:lpips-vgg:2') == ('random:lpips-vgg:2', 'random:lpips-vgg:2')
    assert not (tmp_path / 'o').exists()


def test_tool_usage_errors(tmp_path):
    from click.testing import CliRunner
    tool = _tool()
    a = _images(tmp_path / 'a', [(16, 16), (16, 16)])
    b = _images(tmp_path / 'b', [(16, 16), (16, 12)])
    small = _images(tmp_path / 'small', [(10, 16)])
    three = _images(tmp_path / 'three', [(16, 16)] * 3)
    empty = str(tmp_path / 'empty')
    os.makedirs(empty)
    run = lambda *args: CliRunner().invoke(tool.main, list(args))  # noqa: E731
    r = run('--ref', a)
    assert r.exit_code == 2 and '--test' in r.output
    r = run('--ref', str(tmp_path / 'nowhere'), '--test', a)
    assert r.exit_code == 2 and '--ref' in r.output and 'not a directory' in r.output
    r = run('--ref', a, '--test', empty)
    assert r.exit_code == 2 and '--test' in r.output and 'no PNG or JPEG files' in r.output
    r = run('--ref', a, '--test', b)
    assert r.exit_code == 2 and os.path.join(b, '1.png') in r.output and os.path.join(a, '1.png') in r.output and 'equal sizes' in r.output
    r = run('--ref', small, '--test', small)
    assert r.exit_code == 2 and '11 x 11' in r.output
    r = run('--ref', a, '--test', a, '--masks', three)
    assert r.exit_code == 2 and '--masks' in r.output and 'one per reference image' in r.output
    r = run('--ref', a, '--test', a, '--masks', b)
    assert r.exit_code == 2 and os.path.join(b, '1.png') in r.output and 'equal sizes' in r.output
    r = run('--ref', a, '--test', a, '--lpips_vgg', 'random:lpips-vgg')
    assert r.exit_code == 2 and '--lpips_lin' in r.output
    r = run('--ref', a, '--test', a, '--lpips_lin', 'random:lpips-vgg:1', '--lpips_vgg', 'random:lpips-vgg:2')
    assert r.exit_code == 2 and 'one seed' in r.output
    r = run('--ref', a, '--test', a, '--batch', '0')
    assert r.exit_code == 2 and '--batch' in r.output
