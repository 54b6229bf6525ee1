"""Snapshot preview grids on the GPU: the grid kernel bit for bit against the reference's save_image_grid
(tests/golden/preview_grid.npz) and against plain torch at full size, its argument checks, the grids a tiny training run writes
against render_grid on that tick's snapshot, training bits with previews on versus off, and the evaluation branch."""
import glob
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
BF16, F32 = torch.bfloat16, torch.float32
GW, GH = 7, 4


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    from sid_lsg_amd import ops
    ops.ensure_workspace('cuda')
    return torch.device('cuda')


def _png_pixels(path):
    import PIL.Image
    return np.asarray(PIL.Image.open(path).convert('RGB'))


def _as_layout(x, layout):
    """[B, 3, H, W] -> the kernel's input of that layout; the padding channels of NHWC-8 hold values that must not be read."""
    if layout == 'nchw':
        return x.contiguous()
    B, _, H, W = x.shape
    y = torch.full((B, H, W, 8), 1e9, device=x.device, dtype=F32)
    y[..., 7] = float('nan')
    y[..., :3] = x.permute(0, 2, 3, 1)
    return y


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunks', [(28,), (1,) * 28, (8, 8, 8, 4), (5, 23)], ids=['one-call', 'by-1', 'by-8', '5+23'])
@pytest.mark.parametrize('drange,key', [((-1, 1), 'grid_m1_1'), ((0, 255), 'grid_0_255')], ids=['m1_1', '0_255'])
@pytest.mark.parametrize('layout', ['nhwc8', 'nchw'])
def test_grid_kernel_matches_the_reference_bit_for_bit(dev, golden_dir, layout, drange, key, chunks):
    from sid_lsg_amd import ops
    g = np.load(os.path.join(golden_dir, 'preview_grid.npz'))
    images = torch.from_numpy(g['images']).to(dev)
    want = torch.from_numpy(g[key])
    tile = images.shape[-1]
    grid = torch.full((GH * tile, GW * tile, 3), 77, dtype=torch.uint8, device=dev)
    first = 0
    for n in chunks:
        ops.image_grid_u8(_as_layout(images[first:first + n], layout), grid, first, GW, drange, layout=layout)
        first += n
    assert first == GW * GH
    got = grid.cpu()
    diff = (got != want)
    print(f'{layout} {drange} {chunks[:4]}: {int(diff.sum())} of {diff.numel()} bytes differ')
    assert torch.equal(got, want)


def test_grid_kernel_matches_torch_at_full_size(dev):
    from sid_lsg_amd import ops
    H = W = 512
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(GW * GH, 3, H, W, device=dev, generator=gen) * 0.7
    x[0, 0, 0, :256] = ((torch.arange(256, dtype=torch.float64) + 0.5) / 127.5 - 1.0).to(F32).to(dev)      # lands on ties
    x[1, 1, 5, :4] = torch.tensor([float('inf'), float('-inf'), 0.0, -0.0], device=dev)
    lo, hi = -1, 1
    v = ((x - lo) * (255 / (hi - lo))).round().clamp(0, 255).to(torch.uint8)       # two fp32 kernels, round half to even
    want = v.reshape(GH, GW, 3, H, W).permute(0, 3, 1, 4, 2).reshape(GH * H, GW * W, 3)
    for layout in ('nhwc8', 'nchw'):
        grid = torch.zeros((GH * H, GW * W, 3), dtype=torch.uint8, device=dev)
        src = _as_layout(x, layout)
        for first in range(0, GW * GH, 8):
            ops.image_grid_u8(src[first:first + 8], grid, first, GW, (lo, hi), layout=layout)
        assert torch.equal(grid, want), f'{layout}: {int((grid != want).sum())} bytes differ'


def test_grid_kernel_argument_checks_leave_the_grid_untouched(dev):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    src = torch.zeros(4, 3, 16, 16, device=dev)
    grid = torch.full((GH * 16, GW * 16, 3), 7, dtype=torch.uint8, device=dev)
    fn, sp, gp, st = lib.sidlsg_image_grid_u8.raw, src.data_ptr(), grid.data_ptr(), torch.cuda.current_stream().cuda_stream
    for args in ((sp, gp, 4, 16, 16, 1, 25, GW, GH, -1.0, 1.0),             # first + B > gw * gh
                 (sp, gp, 4, 16, 16, 1, 0, GW, GH, 0.5, 0.5),               # hi == lo
                 (None, gp, 4, 16, 16, 1, 0, GW, GH, -1.0, 1.0), (sp, None, 4, 16, 16, 1, 0, GW, GH, -1.0, 1.0),
                 (sp, gp, 1, 1024, 1024, 1, 0, 32, 32, -1.0, 1.0)):         # a grid of 3 GiB
        assert fn(*args, st) == -22, args
    with pytest.raises(RuntimeError):
        ops.image_grid_u8(src, grid, 25, GW)
    with pytest.raises(RuntimeError):
        ops.image_grid_u8(src, grid, 0, GW, (1, 1))
    with pytest.raises(RuntimeError):
        ops.image_grid_u8(src.cpu(), grid, 0, GW)
    torch.cuda.synchronize()
    assert bool((grid == 7).all())
    # documented, not pinned by numpy: NaN is written as 0
    src[0, 0, 0, 0] = float('nan')
    ops.image_grid_u8(src, grid, 0, GW)
    assert int(grid[0, 0, 0]) == 0 and int(grid[0, 1, 0]) == 128


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def test_training_run_writes_the_grids_of_its_snapshots(dev, tmp_path):
    """3 ticks of one iteration with a snapshot at each: fakes_init.png and fakes_*_{1,2,4}.png per snapshot tick, each equal to
    render_grid on the weights that tick pickled.  (Runs this short name every tick's files alike -- kimg 0 --, so the files of
    tick k are copied away when iteration k + 1 reports.)"""
    from preview_loop_worker import BATCH, ITERATIONS, RESOLUTION, loop_kwargs, write_prompts
    from sid_lsg_amd import preview
    from sid_lsg_amd.data import PromptDataset
    from sid_lsg_amd.sd_util import load_sd15
    from sid_lsg_amd.training_loop import training_loop
    pdir, run = tmp_path / 'prompts', tmp_path / 'run'
    write_prompts(str(pdir))
    run.mkdir()
    names = [f'fakes_1.000000_000000_{n}.png' for n in (1, 2, 4)]

    def keep(tick):
        d = tmp_path / f'tick{tick}'
        d.mkdir()
        for f in names + ['network-snapshot-1.000000-000000.pkl']:
            shutil.copy(run / f, d / f)

    def observer(it, lf, lg):
        if it == 0:
            assert (run / 'fakes_init.png').is_file() and not glob.glob(str(run / 'fakes_1*'))
        else:
            keep(it - 1)
    training_loop(on_iteration=observer, **loop_kwargs(run, pdir, dev, snapshot_images=True))
    keep(ITERATIONS - 1)
    assert sorted(os.path.basename(f) for f in glob.glob(str(run / '*.png'))) == sorted(names + ['fakes_init.png'])

    unet0, vae, sched, te, tok = load_sd15('random:tiny', None, dev, BF16)
    lat = RESOLUTION // 8
    grid = preview.setup_snapshot_grid(PromptDataset(str(pdir), resolution=RESOLUTION), RESOLUTION, BATCH, (4, lat, lat), dev)
    assert grid.size == (GW, GH)
    kw = dict(noise_scheduler=sched, text_encoder=te, tokenizer=tok, vae=vae, init_timestep=625, resolution=RESOLUTION)
    init = _png_pixels(run / 'fakes_init.png')
    assert init.shape == (GH * RESOLUTION, GW * RESOLUTION, 3)
    assert np.array_equal(init, preview.render_grid(unet0.eval().requires_grad_(False), grid, 1, **kw).cpu().numpy())
    seen = []
    for tick in range(ITERATIONS):
        with open(tmp_path / f'tick{tick}' / 'network-snapshot-1.000000-000000.pkl', 'rb') as f:
            ema = pickle.load(f)['ema'].to(dev).eval().requires_grad_(False)
        for n, name in zip((1, 2, 4), names):
            got = _png_pixels(tmp_path / f'tick{tick}' / name)
            assert got.shape == (GH * RESOLUTION, GW * RESOLUTION, 3)
            want = preview.render_grid(ema, grid, n, **kw).cpu().numpy()
            assert np.array_equal(got, want), f'tick {tick}, {n} steps: {int((got != want).sum())} bytes differ'
            seen.append(got)
    # the pictures are pictures of different things: the weights move between ticks and the step counts differ
    assert not np.array_equal(seen[0], seen[3]) and not np.array_equal(seen[0], seen[1]) and not np.array_equal(init, seen[6])


def test_previews_leave_the_training_bits_alone(dev, tmp_path):
    """Deterministic mode, one child process per run: per-iteration losses and the final G / G_ema are bit-equal with the
    previews on and off."""
    from preview_loop_worker import write_prompts
    pdir = tmp_path / 'prompts'
    write_prompts(str(pdir))
    res = {}
    for on in ('0', '1'):                   # one after the other: each child ends, within its own time limit, before the next starts
        out, run = tmp_path / f'out{on}.pt', tmp_path / f'run{on}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'preview_loop_worker.py'), str(out), str(run), str(pdir), on],
                           env=dict(os.environ, SIDLSG_DETERMINISTIC='1'), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f'previews {on}: {r.stdout[-2000:]}{r.stderr[-4000:]}'
        assert 'Deterministic mode: on' in r.stdout
        res[on] = torch.load(out)
        assert len(glob.glob(str(run / '*.png'))) == (4 if on == '1' else 0)
    assert res['0']['losses'].numel() == 6 and bool(torch.isfinite(res['0']['losses']).all())
    for k in ('losses', 'G', 'G_ema'):
        assert torch.equal(res['0'][k], res['1'][k]), f'{k} differs between previews off and on'
    assert not torch.equal(res['0']['G'], res['0']['G_ema'])


def test_evaluation_branch_writes_grids_and_keeps_its_metric_values(dev, tmp_path):
    from sid_lsg_amd.dnnlib_util import EasyDict
    from sid_lsg_amd.training_loop import evaluate_network
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    res = 512
    pkl = tmp_path / 'network-snapshot-1.000000-000123.pkl'
    with open(pkl, 'wb') as f:
        pickle.dump(dict(ema=HipUNet2DCondition(CONFIGS['tiny']).materialize(dev, seed=5)), f)
    caps = tmp_path / 'captions.txt'
    caps.write_text('\n'.join(f'evaluation caption {i}' for i in range(11)) + '\n')
    torch.manual_seed(0)
    proj = torch.randn(3 * 16 * 16, 12, device=dev) * 0.01

    def detector(img, return_features=True):             # the stand-in of tests/test_gpu_unet.py's metrics test
        return torch.nn.functional.adaptive_avg_pool2d(img.float(), 16).flatten(1) @ proj
    out = {}
    for on in (False, True):
        run = tmp_path / f'eval{int(on)}' / 'run'
        run.mkdir(parents=True)
        torch.manual_seed(3)            # the 2- and 4-step samplers of the metrics draw from the global generator
        out[on] = evaluate_network(run_dir=str(run), dataset_kwargs=EasyDict(class_name='sid_lsg_amd.data.CaptionDataset', path=str(caps), resolution=res),
                                   network_kwargs=EasyDict(use_fp16=False), device=dev, metrics=['fid_test'], init_timestep=625,
                                   metric_pt_path=detector, metric_open_clip_path=None, pretrained_model_name_or_path='random:tiny',
                                   network_pkl=str(pkl), resolution=res, metric_real_stats=(np.zeros(12), np.eye(12)), metric_num_test=6,
                                   snapshot_images=on, batch_size=8, batch_gpu=8)
        pngs = sorted(os.path.basename(f) for f in glob.glob(str(run / '*.png')))
        assert pngs == ([f'fid_test000123_{n}.png' for n in (1, 2, 4)] if on else [])
        for p in pngs:
            assert _png_pixels(run / p).shape == (GH * res, GW * res, 3)
        assert all(os.path.isfile(run.parent / f'fid_test000123_{n}.txt') for n in (1, 2, 4))
    assert out[False].keys() == out[True].keys() and len(out[True]) == 3
    for k in out[True]:
        a, b = out[False][k].results['fid30k_full'], out[True][k].results['fid30k_full']
        assert np.isfinite(a) and a == b, (k, a, b)
    assert len({out[True][k].results['fid30k_full'] for k in out[True]}) == 3
