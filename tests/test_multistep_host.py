"""Multi-step generator training (--num_steps N > 1), host side: the input stream draws the sampler's eps_i where the reference loop
draws them (tests/golden/loop_ns*.npz, recorded from the UNMODIFIED reference training_loop), the step timesteps, the CLI range."""
import os

import numpy as np
import pytest
import torch

LOOP_GOLDENS = ['loop_ns2_k15_a1', 'loop_ns4_k1_a12', 'loop_v_ns2_k15_a1']


@pytest.mark.parametrize('golden', LOOP_GOLDENS)
def test_prompt_stream_reproduces_the_reference_multistep_draws(golden_dir, tmp_path, golden):
    """PromptStream(num_steps=N) on the CPU generator against the draws the reference loop made in its first iteration: z, noise,
    eps_1 .. eps_{N-1}, t of every round, phase A (eps before t) and phase B (t before eps) -- bit for bit."""
    from oracle import fixtures
    from sid_lsg_amd.data import PromptDataset
    from sid_lsg_amd.training_loop import PromptStream
    g = np.load(os.path.join(golden_dir, golden + '.npz'))
    n = int(g['num_steps'])
    prompts = [str(p) for p in g['prompts']]
    pdir = tmp_path / 'p'
    pdir.mkdir()
    (pdir / 'aesthetics_6_plus.txt').write_text('\n'.join(prompts) + '\n')
    res, bs, bg = int(g['kw_resolution']), int(g['kw_batch_size']), int(g['kw_batch_gpu'])
    ds = PromptDataset(str(pdir), resolution=res)
    fixtures.factory(str(g['cfg']))           # (module construction consumes RNG: before the stream is seeded, as in the loop)
    stream = PromptStream(ds, seed=int(g['kw_seed']), rank=0, world=1, batch_gpu=bg, lat=res // 8, tmin=20, tmax=980, device='cpu',
                          rng_device='cpu', num_steps=n)
    for _ in range(16):
        stream.next_prompts()
    kappa = [float(k) for k in g['kw_kappa']]
    use_dropout = kappa[0] != 1 or kappa[1] != 1
    for ph, drop in (('A', use_dropout), ('B', False)):
        for r in range(bs // bg):
            ps, z, noise, t, eps = stream.round(drop, ph)
            assert eps.shape == (n - 1,) + tuple(z.shape)
            assert torch.equal(z, torch.from_numpy(g[f'draw_{ph}_z'][r])), (ph, r, 'z')
            assert torch.equal(noise, torch.from_numpy(g[f'draw_{ph}_noise'][r])), (ph, r, 'noise')
            assert torch.equal(eps, torch.from_numpy(g[f'draw_{ph}_eps'][r])), (ph, r, 'eps')
            assert torch.equal(t, torch.from_numpy(g[f'draw_{ph}_t'][r])), (ph, r, 't')


def test_one_step_stream_is_unchanged(tmp_path):
    """num_steps = 1 (the default): the same 4-tuple and the same draws as before the option existed."""
    from sid_lsg_amd.data import PromptDataset
    from sid_lsg_amd.training_loop import PromptStream
    pdir = tmp_path / 'p'
    pdir.mkdir()
    (pdir / 'aesthetics_6_plus.txt').write_text('\n'.join(f'prompt {i}' for i in range(8)) + '\n')
    ds = PromptDataset(str(pdir), resolution=64)
    # (a stream seeds the process-wide generators: one stream at a time)
    a = PromptStream(ds, seed=1, rank=0, world=1, batch_gpu=2, lat=8, tmin=20, tmax=980, device='cpu', rng_device='cpu')
    ra = [a.round(False) for _ in range(2)]
    b = PromptStream(ds, seed=1, rank=0, world=1, batch_gpu=2, lat=8, tmin=20, tmax=980, device='cpu', rng_device='cpu', num_steps=1)
    rb = [b.round(False, ph) for ph in ('A', 'B')]
    for x, y in zip(ra, rb):
        assert len(x) == len(y) == 4
        assert x[0] == y[0] and all(torch.equal(u, v) for u, v in zip(x[1:], y[1:]))
    with pytest.raises(ValueError):
        PromptStream(ds, seed=1, rank=0, world=1, batch_gpu=2, lat=8, tmin=20, tmax=980, device='cpu', num_steps=0)
    with pytest.raises(ValueError):
        a.round(False, 'C')


def test_step_timesteps_truncate_like_the_reference():
    """t_i = (init_t * (1 - i/N)).long(): N = 2 -> 625, 312; N = 4 -> 625, 468, 312, 156 (sid_sd_util.py:178)."""
    from sid_lsg_amd.sd_util import step_timesteps
    init_t = torch.full((3,), 625, dtype=torch.long)
    assert [int(t[0]) for t in step_timesteps(init_t, 1)] == [625]
    assert [int(t[0]) for t in step_timesteps(init_t, 2)] == [625, 312]
    assert [int(t[0]) for t in step_timesteps(init_t, 4)] == [625, 468, 312, 156]
    assert all(t.dtype == torch.long and t.shape == (3,) for t in step_timesteps(init_t, 4))


def test_cli_num_steps_range():
    """sid_train.py --num_steps takes N >= 1; 0 is refused by the option parser."""
    import click
    import sid_train
    opt = {f[0]: kw for f, kw in sid_train.OPTIONS}['--num_steps']
    assert isinstance(opt['type'], click.IntRange) and opt['type'].min == 1
    with pytest.raises(click.BadParameter):
        opt['type'].convert('0', None, None)
    assert opt['type'].convert('4', None, None) == 4
