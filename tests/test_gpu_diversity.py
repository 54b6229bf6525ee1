"""Per-prompt diversity on the GPU: sidlsg_lpips_group_f32 bit for bit against the paired kernel on the gathered pair list and against
fp64 (inputs and preconditions: tests/diversity_cases.py), its refusals, HipLPIPS.group_pairs against HipLPIPS on single pairs, the
two command lines against each other, and the lpipsdiv_test metric."""
import importlib.util
import json
import math
import os
from functools import partial

import numpy as np
import pytest
import torch

import diversity_cases as dc
import inception_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
LP = ['--lpips_vgg', 'random:lpips-vgg:1', '--lpips_lin', 'random:lpips-vgg:1']


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def _paired(F, w, G, K, dev):
    """The paired kernel on the gathered pair list -> [G, P] on the host."""
    from sid_lsg_amd import fidelity
    return fidelity.lpips_layer_f32(dc.gather(F, G, K).to(dev), w.to(dev)).cpu().reshape(G, -1)


# ---- 1. the kernel against the paired kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', dc.BIT_CASES + dc.EXTRA_BIT_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_group_layer_is_bit_equal_to_the_paired_kernel(dev, case):
    """Every pair of every group has the bits sidlsg_lpips_layer_f32 writes for it, in the form the library picks by the size of the
    map and in each of its two launch forms by name (all pairs of a pixel block in one workgroup; one workgroup per block and pair).
    Precondition: the paired kernel's values of the case are pairwise distinct, so a permuted or repeated pair index cannot pass."""
    from sid_lsg_amd import fidelity
    C, ldf, h, wd, G, K = case
    F, w = dc.make(case)
    want = _paired(F, w, G, K, dev)
    flat = want.reshape(-1).tolist()
    assert len(set(flat)) == len(flat) == G * K * (K - 1) // 2 and all(math.isfinite(v) and v > 0 for v in flat), 'precondition: distinct values'
    got = fidelity.lpips_group_f32(F.to(dev), w.to(dev), K)
    assert got.dtype == torch.float64 and tuple(got.shape) == (G, K * (K - 1) // 2)
    worst = float((got.cpu() - want).abs().max())
    print(f'lpips_group {case}: values {min(flat):.6g} .. {max(flat):.6g}, max |group - paired| {worst:.3g}')
    assert torch.equal(got.cpu(), want)
    for form in dc.forms(C, K)[1:]:
        named = fidelity.lpips_group_f32(F.to(dev), w.to(dev), K, form=form).cpu()
        assert torch.equal(named, want), form
        assert torch.equal(fidelity.lpips_group_f32(F.to(dev), w.to(dev), K, form=form).cpu(), named), form          # the same inputs give the same bits
    if not dc.chip_fits(C, K):                                     # refused by name, not run in another form
        with pytest.raises(RuntimeError, match='sidlsg_lpips_group_form_f32'):
            fidelity.lpips_group_f32(F.to(dev), w.to(dev), K, form='chip')


def test_planted_identical_pair_is_exactly_zero(dev):
    """(20, 32, 16, 17, 3, 5) with row 3 of group 1 planted equal to row 1 of that group: the pair (1, 3) is exactly 0, everything is
    still the paired kernel's bits, and the values are distinct apart from the planted zero and the pairs of the copy, which
    necessarily repeat those of the row it copies."""
    from sid_lsg_amd import fidelity
    case = (20, 32, 16, 17, 3, 5)
    C, ldf, h, wd, G, K = case
    F, w = dc.make(case)
    F = F.clone()
    F[1 * K + 3] = F[1 * K + 1]
    want = _paired(F, w, G, K, dev)
    got = fidelity.lpips_group_f32(F.to(dev), w.to(dev), K, form='chip').cpu()
    table = dc.pair_table(K)
    assert got[1, table.index((1, 3))] == 0.0 and torch.equal(got, want)
    assert torch.equal(fidelity.lpips_group_f32(F.to(dev), w.to(dev), K, form='pairs').cpu(), want)
    keep = [v for g in range(G) for (i, j), v in zip(table, want[g].tolist()) if not (g == 1 and 3 in (i, j))]
    assert len(set(keep)) == len(keep) and all(v > 0 for v in keep)
    for other in (0, 2, 4):                                        # the copy's pairs: the original's, bit for bit
        a, b = table.index(tuple(sorted((1, other)))), table.index(tuple(sorted((3, other))))
        assert got[1, a] == got[1, b] and got[1, a] > 0


@pytest.mark.parametrize('shape,G,K', [((20, 32, 16, 17), 3, 5), ((64, 64, 7, 9), 2, 16)], ids=['K5', 'K16'])
def test_a_pair_does_not_depend_on_G_K_or_position(dev, shape, G, K):
    """One pair of rows as rows (0, 1) of a K = 2 group, and as rows (1, 3) of the last group of a larger buffer whose other rows are
    filled by the recipe: the same bits, in every launch form.  In the on-chip form the second case crosses from a workgroup of 256
    threads (K = 2) to one of 128 (K = 16)."""
    from sid_lsg_amd import fidelity
    C, ldf, h, wd = shape
    gen = torch.Generator().manual_seed(C + h + K)
    pair = dc.rows(C, ldf, h, wd, 1, 2, gen, first_group=1)
    big = dc.rows(C, ldf, h, wd, G, K, gen)
    w = (0.1 * torch.rand(C, generator=gen)).to(dev)
    big[(G - 1) * K + 1], big[(G - 1) * K + 3] = pair[0], pair[1]
    paired = fidelity.lpips_layer_f32(pair.to(dev), w).cpu()
    for form in ('chip', 'pairs', None):
        alone = fidelity.lpips_group_f32(pair.to(dev), w, 2, form=form).cpu()
        inside = fidelity.lpips_group_f32(big.to(dev), w, K, form=form).cpu()
        assert tuple(alone.shape) == (1, 1) and alone[0, 0] > 0, form
        assert alone[0, 0] == paired[0] and inside[G - 1, dc.pair_table(K).index((1, 3))] == alone[0, 0], form


def test_all_zero_pixels_contribute_zero(dev):
    """A pixel that is all zero contributes 0 (0 / (0 + 1e-10) = 0): maps of zeros give exactly 0 for every pair, and with a pixel
    dead in all three rows of a group the values are still the paired kernel's bits (the recipe's dead pixels are per row)."""
    from sid_lsg_amd import fidelity
    w = (0.1 * torch.rand(64, generator=torch.Generator().manual_seed(0))).to(dev)
    zeros = torch.zeros(3, 9, 15, 64, device=dev)
    for form in ('chip', 'pairs'):
        assert fidelity.lpips_group_f32(zeros, w, 3, form=form).tolist() == [[0.0, 0.0, 0.0]], form
    F, _ = dc.make((64, 64, 7, 9, 2, 3))
    one = F[:3].clone()
    one[:, 0, 0] = 0.0                                              # pixel (0, 0) dead in all three rows
    got = fidelity.lpips_group_f32(one.to(dev), w, 3, form='chip').cpu()
    want = fidelity.lpips_layer_f32(dc.gather(one, 1, 3).to(dev), w).cpu().reshape(1, 3)
    assert torch.equal(got, want) and bool((got > 0).all())


# ---- 2. against fp64 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', dc.FP64_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_group_layer_against_fp64(dev, case):
    """|got - want| <= k(C) 2^-24 M with want and M from fidelity_ref.lpips_layer on the gathered pairs and k(C) = 2 * 4 ceil(C / 64) + 18,
    the derivation of tests/test_gpu_fidelity.py::test_lpips_layer_against_fp64: the rounding sequence is the paired kernel's.
    Precondition: any two different pairs' fp64 values differ by at least 4 x the larger of their bounds, so a value that lands in
    another pair's slot exceeds the bound (960, 13.6 and 12.3 times the bound for the three cases; the K = 16 cases have 0.4 and 3.8
    and appear in the bit-equality test only)."""
    from sid_lsg_amd import fidelity
    C, ldf, h, wd, G, K = case
    F, w = dc.make(case)
    want, M = dc.fp64(case)
    gap = dc.smallest_gap(case)
    assert gap >= 4, f'precondition: smallest gap {gap} x the bound'
    for form in dc.forms(C, K):
        got = fidelity.lpips_group_f32(F.to(dev), w.to(dev), K, form=form).cpu()
        ratio = (got - want).abs() / (dc.k_bound(C) * dc.U * M)
        print(f'lpips_group {case} form {form}: smallest gap between pairs {gap:.1f} x the bound; error / bound, max {float(ratio.max()):.3g} (k = {dc.k_bound(C)})')
        assert bool(torch.isfinite(got).all()) and bool((ratio <= 1).all()), form


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------------
def test_group_layer_refusals(dev):
    from sid_lsg_amd import fidelity
    from sid_lsg_amd._lib import lib
    F = torch.zeros(4, 2, 2, 8, device=dev)
    w = torch.zeros(8, device=dev)
    out = torch.full((6,), -1.0, dtype=torch.float64, device=dev)
    ws = torch.empty(64, dtype=torch.float64, device=dev)
    pf, pw, po, pws = F.data_ptr(), w.data_ptr(), out.data_ptr(), ws.data_ptr()

    def call(pf=pf, ldf=8, pw=pw, G=1, K=4, C=8, po=po, pws=pws, h=2, wd=2):
        rcs = {lib.sidlsg_lpips_group_f32.raw(pf, ldf, pw, G, K, h, wd, C, po, pws, None)}
        rcs |= {lib.sidlsg_lpips_group_form_f32.raw(pf, ldf, pw, G, K, h, wd, C, form, po, pws, None) for form in (0, 1, 2)}
        assert len(rcs) == 1, rcs                                   # the named forms refuse what the plain entry point refuses
        return rcs.pop()
    size = lib.sidlsg_lpips_group_ws_doubles.raw
    assert call(K=1) == EINVAL and call(K=17) == EINVAL and call(G=0) == EINVAL
    assert size(1, 1, 2, 2) < 0 and size(1, 17, 2, 2) < 0 and size(0, 4, 2, 2) < 0
    assert call(C=6) == EINVAL and call(ldf=4) == EINVAL and call(C=0) == EINVAL and call(ldf=10, C=8) == EINVAL
    assert call(pf=pf + 4) == EINVAL and call(pw=pw + 4) == EINVAL and call(po=po + 4) == EINVAL and call(pws=pws + 4) == EINVAL
    assert call(pf=None) == EINVAL and call(pw=None) == EINVAL and call(po=None) == EINVAL and call(pws=None) == EINVAL
    assert call(G=5462, K=4) == EINVAL and size(5462, 4, 2, 2) < 0            # G P = 32772 pairs
    assert call(G=2048, K=16) == EINVAL and size(2048, 16, 2, 2) < 0          # G K = 32768 maps
    assert call(G=1, K=4, h=4096, wd=4096 * 4) == EINVAL                      # F of 2^31 bytes and more
    assert call(h=0) == EINVAL and size(1, 4, 0, 2) < 0
    for form in (-1, 3):
        assert lib.sidlsg_lpips_group_form_f32.raw(pf, 8, pw, 1, 4, 2, 2, 8, form, po, pws, None) == EINVAL
    big = torch.zeros(16, 1, 1, 512, device=dev)                   # the on-chip form by name where K vectors of C = 512 do not fit in LDS
    w512 = torch.zeros(512, device=dev)
    pb, pw512 = big.data_ptr(), w512.data_ptr()
    assert [lib.sidlsg_lpips_group_form_f32.raw(pb, 512, pw512, 1, K, 1, 1, 512, 1, po, pws, None) for K in (3, 4, 16)] == [0, EINVAL, EINVAL]
    torch.cuda.synchronize()
    assert out[:3].tolist() == [0.0, 0.0, 0.0] and bool((out[3:] == -1).all())          # K = 3 ran (maps of zeros), the others did not
    out.fill_(-1.0)
    assert size(3, 5, 16, 17) == 3 * 10 * 3 and size(1, 16, 2, 3) == 120 and size(5461, 4, 2, 2) == 5461 * 6
    torch.cuda.synchronize()
    assert bool((out == -1).all())                                 # nothing was launched
    with pytest.raises(RuntimeError, match='groups of 3'):
        fidelity.lpips_group_f32(F, w, 3)
    with pytest.raises(RuntimeError, match='admitted set'):
        fidelity.lpips_group_f32(torch.zeros(17, 2, 2, 8, device=dev), w, 17)
    with pytest.raises(RuntimeError):
        fidelity.lpips_group_f32(F.cpu(), w.cpu(), 2)


# ---- 4. HipLPIPS.group_pairs -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hip(dev):
    from sid_lsg_amd import fidelity
    return fidelity.load_lpips('random:lpips-vgg', 'random:lpips-vgg', dev)


def _count_launches(monkeypatch, fn):
    """fn() with every entry point of the library counted -> (result, {name: calls}) (tests/test_gpu_fidelity.py's pattern)."""
    from sid_lsg_amd._lib import lib
    counts = {}
    for name in lib.protos:
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*a)
        counted.raw = real.raw
        monkeypatch.setitem(lib.__dict__, name, counted)
    out = fn()
    monkeypatch.undo()
    return out, counts


@pytest.mark.parametrize('G,H,W', [(2, 32, 32), (1, 40, 56)])
def test_group_pairs_equals_single_pairs(dev, hip, monkeypatch, G, H, W):
    from sid_lsg_amd import fidelity
    K = 3
    x = inception_ref.structured_images(G * K, H, W, seed=H + G).to(dev)
    got, counts = _count_launches(monkeypatch, lambda: hip.group_pairs(x, K))
    assert counts == {'sidlsg_lpips_input_u8': 1, 'sidlsg_conv2d_relu_f32': 13, 'sidlsg_pool2d_f32': 4, 'sidlsg_lpips_group_f32': 5,
                      'sidlsg_lpips_sum_f64': 1}, counts
    assert got.dtype == torch.float64 and tuple(got.shape) == (G, 3)
    want = torch.stack([torch.cat([hip(x[g * K + i][None], x[g * K + j][None]) for i, j in dc.pair_table(K)]) for g in range(G)])
    print(f'group_pairs {G} x {K} of {H} x {W}: {got.tolist()}')
    assert torch.equal(got, want) and bool((got > 1e-3).all()) and len(set(got.reshape(-1).tolist())) == G * 3
    # the maps of `features` are the bits `taps` gives an image, for an even and for an odd count
    for n in (G * K, G * K - 1) if G > 1 else (G * K,):
        feats = [f.clone() for f in hip.features(x[:n])]
        taps = [f.clone() for f in hip.taps(x[:1], x[n - 1:n])]
        assert all(f.shape[0] == n and torch.equal(f[0], t[0]) and torch.equal(f[n - 1], t[1]) for f, t in zip(feats, taps))
    # a group of identical images: all zeros
    same = x[:1].repeat(K, 1, 1, 1)
    assert hip.group_pairs(same, K).tolist() == [[0.0, 0.0, 0.0]]
    if G > 1:
        # chunked by whole groups: one group fits per pass
        monkeypatch.setattr(fidelity.HipLPIPS, 'max_pairs', staticmethod(lambda H, W: 2))
        chunked, counts = _count_launches(monkeypatch, lambda: hip.group_pairs(x, K))
        assert counts['sidlsg_lpips_input_u8'] == 2 and counts['sidlsg_lpips_group_f32'] == 10 and counts['sidlsg_lpips_sum_f64'] == 2, counts
        assert torch.equal(chunked, got)
        # a K larger than a pass is refused by name
        monkeypatch.setattr(fidelity.HipLPIPS, 'max_pairs', staticmethod(lambda H, W: 1))
        with pytest.raises(ValueError, match=f'K = 3 images of {H} x {W} exceeds one pass'):
            hip.group_pairs(x, K)


def test_group_pairs_refusals(dev, hip):
    x = inception_ref.structured_images(4, 16, 24, seed=1).to(dev)
    with pytest.raises(ValueError, match='too small'):
        hip.group_pairs(x[:, :, :12, :12].contiguous(), 2)
    with pytest.raises(ValueError, match='whole groups'):
        hip.group_pairs(x, 3)
    with pytest.raises(ValueError, match='2 <= K <= 16'):
        hip.group_pairs(x, 1)
    with pytest.raises(RuntimeError):
        hip.group_pairs(x.float(), 2)
    assert tuple(hip.group_pairs(x, 4).shape) == (1, 6) and tuple(hip.group_pairs(x, 2).shape) == (2, 1)


# ---- 5. command lines -------------------------------------------------------------------------------------------------------------------------
def _png(path):
    import PIL.Image
    return torch.from_numpy(np.asarray(PIL.Image.open(path).convert('RGB')).transpose(2, 0, 1).copy())


def test_generate_onestep_diversity_equals_the_tool(dev, tmp_path, monkeypatch):
    """--seeds_per_prompt 3 --diversity 1 on the teacher: diversity.json holds groups 0 and 1 with the right prompts and files; its pair
    values are HipLPIPS on the PNG pairs read back; tools/prompt_diversity.py on the folder prints the same figures.  Files 0-2 are
    byte-identical to those of a run with --seeds_per_prompt 1 and a prompt file holding the first prompt alone (the option changes
    the condition index and nothing else), and a run without the option writes the files of a run with the option given as 1."""
    from click.testing import CliRunner
    import generate_onestep
    from sid_lsg_amd import fidelity
    monkeypatch.setattr(fidelity, '_warned', set())                # the once-per-process notice: this test's own record of it
    spec = importlib.util.spec_from_file_location('prompt_diversity', os.path.join(ROOT, 'tools', 'prompt_diversity.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    prompts, first = tmp_path / 'prompts.txt', tmp_path / 'first.txt'
    prompts.write_text('a red cube\na blue sphere\n')
    first.write_text('a red cube\n')
    base = ['--network', 'teacher', '--repo_id', 'random:tiny', '--teacher_steps', '2', '--guidance_scale', '2', '--resolution', '64', '--batch', '4']

    def run(out, *args):
        r = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out), *base, *args], catch_exceptions=False)
        assert r.exit_code == 0, r.output
        return r.output
    out = tmp_path / 'out'
    text = run(out, '--seeds', '0-5', '--seeds_per_prompt', '3', '--text_prompts', str(prompts), '--diversity', '1', *LP)
    assert 'Diversity over 2 groups' in text and 'not comparable' in text
    with open(out / 'diversity.json') as f:
        report = json.load(f)
    assert sorted(report) == ['mean', 'options', 'per_prompt'] and sorted(report['per_prompt']) == ['0', '1']
    assert report['options']['seeds_per_prompt'] == 3 and report['options']['lpips_vgg'] == 'random:lpips-vgg:1'
    assert report['per_prompt']['0']['prompt'] == 'a red cube' and report['per_prompt']['1']['prompt'] == 'a blue sphere'
    assert report['per_prompt']['0']['files'] == ['000000.png', '000001.png', '000002.png']
    assert report['per_prompt']['1']['files'] == ['000003.png', '000004.png', '000005.png']
    assert sorted(f for f in os.listdir(out) if f.endswith('.png')) == [f'{i:06d}.png' for i in range(6)]
    net = fidelity.load_lpips(LP[1], LP[3], dev)
    for g in ('0', '1'):
        row = report['per_prompt'][g]
        assert sorted(row) == sorted(('prompt', 'files', 'lpips', 'lpips_min', 'lpips_pairs', 'ssim', 'mse'))
        imgs = [_png(out / name).to(dev) for name in row['files']]
        want = [float(net(imgs[i][None], imgs[j][None])[0]) for i, j in dc.pair_table(3)]
        assert row['lpips_pairs'] == want and all(v > 0 for v in want)
        assert row['lpips'] == ((want[0] + want[1]) + want[2]) / 3 and row['lpips_min'] == min(want)
        assert 0 < row['ssim'] < 1 and row['mse'] > 0
    mean = report['mean']
    assert mean['groups'] == 2 and mean['lpips'] == (report['per_prompt']['0']['lpips'] + report['per_prompt']['1']['lpips']) / 2
    assert mean['lpips_std'] == pytest.approx(abs(report['per_prompt']['0']['lpips'] - report['per_prompt']['1']['lpips']) / 2, rel=1e-12)
    # the stand-alone tool on the written files, in one call for both groups and one group per call
    for batch in ('6', '1'):
        r = CliRunner().invoke(tool.main, ['--images', str(out), '--group', '3', '--prompts', str(prompts), '--batch', batch, *LP], catch_exceptions=False)
        assert r.exit_code == 0, r.output
        again = json.loads(r.output[r.output.index('{'):])
        assert again['per_prompt'] == report['per_prompt'] and again['mean'] == report['mean']
    # the option changes the condition index and nothing else
    one = tmp_path / 'one'
    run(one, '--seeds', '0-2', '--seeds_per_prompt', '1', '--text_prompts', str(first))
    for i in range(3):
        assert (one / f'{i:06d}.png').read_bytes() == (out / f'{i:06d}.png').read_bytes(), i
    assert not (one / 'diversity.json').exists()
    # without the option: the files of a run with the option given as 1
    plain, given = tmp_path / 'plain', tmp_path / 'given'
    run(plain, '--seeds', '0-3', '--text_prompts', str(prompts))
    run(given, '--seeds', '0-3', '--text_prompts', str(prompts), '--seeds_per_prompt', '1')
    assert sorted(os.listdir(plain)) == sorted(os.listdir(given)) == [f'{i:06d}.png' for i in range(4)]
    for i in range(4):
        assert (plain / f'{i:06d}.png').read_bytes() == (given / f'{i:06d}.png').read_bytes(), i
    assert (plain / '000001.png').read_bytes() != (out / '000001.png').read_bytes()          # sample 1: prompt 1 there, prompt 0 under K = 3


# ---- 6. the metric -----------------------------------------------------------------------------------------------------------------------------
def test_lpipsdiv_test_metric(dev, monkeypatch):
    from sid_lsg_amd import fidelity, metrics
    monkeypatch.setattr(fidelity, '_warned', set())                # the once-per-process notice: this test's own record of it
    from sid_lsg_amd.sd_util import load_sd15, sid_sd_sampler
    unet, vae, sched, te, tok = load_sd15('random:tiny', None, dev, torch.bfloat16)
    unet.eval().requires_grad_(False)
    G = partial(sid_sd_sampler, unet=unet, noise_scheduler=sched, text_encoder=te, tokenizer=tok, resolution=64, dtype=torch.float32,
                return_images=True, vae=vae, train_sampler=False)
    seen = []

    def G_rec(latents, contexts, init_timesteps):
        seen.append(list(contexts))
        return G(latents=latents, contexts=contexts, init_timesteps=init_timesteps)
    kw = dict(G=G_rec, prompts=['a red cube', 'blue sphere', 'two cats'], resolution=64, init_timestep=625, device=dev, num_test=2, batch_gen=3)
    spec = dict(metric_lpips_vgg='random:lpips-vgg:1', metric_lpips_lin='random:lpips-vgg:1')
    res = metrics.calc_metric('lpipsdiv_test', **kw, **spec).results
    assert sorted(res) == ['lpipsdiv_test', 'lpipsdiv_test_min']
    print(f'lpipsdiv_test {res.lpipsdiv_test}, min {res.lpipsdiv_test_min}')
    assert math.isfinite(res.lpipsdiv_test) and res.lpipsdiv_test > 0 and 0 < res.lpipsdiv_test_min <= res.lpipsdiv_test
    # 2 prompts x 4 seeds in batches of 3 + 1, every batch under one prompt
    assert [len(c) for c in seen] == [3, 1, 3, 1] and all(len(set(c)) == 1 for c in seen) and seen[0][0] == seen[1][0] != seen[2][0]
    again = metrics.calc_metric('lpipsdiv_test', **kw, **spec).results
    assert again == res
    with pytest.raises(ValueError, match='--metric_lpips_vgg.*--metric_lpips_lin'):
        metrics.calc_metric('lpipsdiv_test', **kw)
    with pytest.raises(ValueError, match='metric_lpips_lin|lpips_lin'):
        metrics.calc_metric('lpipsdiv_test', **kw, metric_lpips_vgg='random:lpips-vgg:1')
