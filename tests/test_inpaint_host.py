"""Host side of inpainting and of image-to-image with the teacher: the entry rule (teacher_start_index), the `start` argument of the
solver tables, the mask loader and the 'any pixel of the 8 x 8 block' latent rule, the pixel composite and the option helpers of
generate_onestep.py.  No GPU."""
import math

import numpy as np
import pytest
import torch

SD = dict(steps_offset=1, set_alpha_to_one=False, timestep_spacing='leading')


def _sched():
    from sid_lsg_amd.scheduler import DDPMScheduler
    return DDPMScheduler()


def test_teacher_start_index_is_the_img2img_rule():
    from sid_lsg_amd.sd_util import teacher_start_index
    for n, s, k in ((50, 0.8, 10), (10, 0.3, 7), (100, 0.29, 72), (4, 1.0, 0)):
        assert teacher_start_index(n, s) == k, (n, s, k)
    assert int(10 * 0.3) == 3 and int(100 * 0.29) == 28             # N*S is formed in floating point, as diffusers forms it
    with pytest.raises(ValueError, match='strength'):
        teacher_start_index(10, 0.05)
    with pytest.raises(ValueError):
        teacher_start_index(0, 0.5)


def test_solver_tables_start_selects_the_first_order_row():
    """dpmpp2m, N = 5, start = 2: row 2 is (sigma_t/sigma_s, alpha_t*(1 - exp(-h)), 0, 0) from an fp64 restatement, within 2 fp32 ulps
    after solver_schedule's rounding (the bound of tests/test_solver_host.py for the tables); everything else has the bits of start=0."""
    from sid_lsg_amd.scheduler import solver_schedule, solver_tables
    sched, N, k = _sched(), 5, 2
    base = solver_tables(sched, SD, N, 'dpmpp2m', 'leading')
    same = solver_tables(sched, SD, N, 'dpmpp2m', 'leading', start=0)
    got = solver_tables(sched, SD, N, 'dpmpp2m', 'leading', start=k)
    for a, b in zip(base, same):
        assert np.array_equal(a, b)
    for a, b in zip(base[:3], got[:3]):                              # timesteps, alpha, sigma
        assert np.array_equal(a, b)
    others = [i for i in range(N) if i != k]
    assert np.array_equal(base[3][others], got[3][others])
    assert base[3][k, 2] != 0 and got[3][k, 2] == 0 and got[3][k, 3] == 0
    # the fp64 restatement, from the scheduler's own fp32 alphas_cumprod
    abar = sched.alphas_cumprod.double().numpy()
    t = got[0]
    a_s, a_t = float(abar[t[k]]), float(abar[t[k + 1]])
    lam = lambda a: 0.5 * (math.log(a) - math.log1p(-a))  # noqa: E731
    h = lam(a_t) - lam(a_s)
    want = (math.sqrt(1 - a_t) / math.sqrt(1 - a_s), math.sqrt(a_t) * (1 - math.exp(-h)), 0.0, 0.0)
    ts32, s0, s1, coef = solver_schedule(sched, SD, N, 'dpmpp2m', 'leading', start=k)
    for j in range(4):
        ulp = float(np.spacing(np.float32(abs(want[j])))) if want[j] != 0 else 0.0
        assert abs(float(coef[k, j]) - want[j]) <= 2 * ulp, (j, float(coef[k, j]), want[j])
    ts0, s00, s10, coef0 = solver_schedule(sched, SD, N, 'dpmpp2m', 'leading')
    assert torch.equal(ts32, ts0) and torch.equal(s0, s00) and torch.equal(s1, s10) and torch.equal(coef[others], coef0[others])
    for a, b in zip(solver_schedule(sched, SD, N, 'dpmpp2m', 'leading', start=0), (ts0, s00, s10, coef0)):
        assert torch.equal(a, b)


def test_solver_tables_start_leaves_ddim_alone_and_is_validated():
    from sid_lsg_amd.scheduler import solver_schedule, solver_tables
    sched, N = _sched(), 5
    base = solver_tables(sched, SD, N, 'ddim', 'trailing', eta=0.5)
    for k in range(N):
        for a, b in zip(base, solver_tables(sched, SD, N, 'ddim', 'trailing', eta=0.5, start=k)):
            assert np.array_equal(a, b)
    for solver in ('ddim', 'dpmpp2m'):
        for bad in (N, N + 3, -1):
            with pytest.raises(ValueError, match='start'):
                solver_tables(sched, SD, N, solver, 'leading', start=bad)
            with pytest.raises(ValueError, match='start'):
                solver_schedule(sched, SD, N, solver, 'leading', start=bad)
    # the last step is the x0 row whatever start is
    assert solver_tables(sched, SD, N, 'dpmpp2m', 'leading', start=N - 1)[3][N - 1].tolist() == [0.0, 1.0, 0.0, 0.0]


def _write_images(d, masks):
    """Init images of 16 x 24, 16 x 16 and 20 x 16 pixels in d/init, the given 'L' masks in d/masks."""
    import PIL.Image
    rng = np.random.default_rng(3)
    (d / 'init').mkdir()
    (d / 'masks').mkdir()
    imgs = {'a.png': rng.integers(0, 256, (16, 24, 3), dtype=np.uint8), 'b.png': rng.integers(0, 256, (16, 16, 3), dtype=np.uint8),
            'c.png': rng.integers(0, 256, (20, 16, 3), dtype=np.uint8)}
    for name, px in imgs.items():
        PIL.Image.fromarray(px, 'RGB').save(d / 'init' / name)
    for name, px in masks.items():
        PIL.Image.fromarray(px, 'L').save(d / 'masks' / name)
    return imgs


def test_mask_loader_crops_as_the_init_image_and_repaints_any_marked_cell(tmp_path):
    import generate_onestep as g
    wide, tall = np.zeros((16, 24), np.uint8), np.zeros((20, 16), np.uint8)
    wide[9, 4 + 10] = 128                    # column 14 of the file is column 10 of the centre crop: latent cell (1, 1)
    wide[3, 2] = 255                         # outside the centre crop: cut away with the init image's margin
    tall[2 + 7, 15] = 128                    # row 9 of the file is row 7 of the crop: latent cell (0, 1)
    tall[2 + 8, 0] = 127                     # below the threshold: repaints nothing
    _write_images(tmp_path, {'m0.png': wide, 'm1.png': np.zeros((16, 16), np.uint8), 'm2.png': tall})
    files = g.list_mask_images(str(tmp_path / 'masks'), 3)
    assert [f.rsplit('/', 1)[1] for f in files] == ['m0.png', 'm1.png', 'm2.png']
    px = g.load_mask_batch(files, [0, 1, 2, 3], 16)
    assert px.shape == (4, 16, 16) and px.dtype == np.uint8
    assert np.array_equal(px[0], wide[:, 4:20]) and np.array_equal(px[2], tall[2:18]) and np.array_equal(px[3], px[0])
    lat = g.latent_mask(px)
    assert lat.shape == (4, 2, 2) and lat.dtype == np.uint8
    assert lat[0].tolist() == [[0, 0], [0, 1]] and lat[1].tolist() == [[0, 0], [0, 0]] and lat[2].tolist() == [[0, 1], [0, 0]]
    # a NEAREST resize keeps the values binary: a 32 x 32 file at resolution 16
    import PIL.Image
    big = np.zeros((32, 32), np.uint8)
    big[16:, :16] = 255
    PIL.Image.fromarray(big, 'L').save(tmp_path / 'big.png')
    small = g.load_mask_image(str(tmp_path / 'big.png'), 16)
    assert set(np.unique(small).tolist()) == {0, 255} and g.latent_mask(small[None])[0].tolist() == [[0, 0], [1, 0]]


def test_one_mask_serves_all_samples_and_counts_are_checked(tmp_path):
    import click
    import generate_onestep as g
    one = np.zeros((16, 16), np.uint8)
    one[0, 0] = 200
    _write_images(tmp_path, {'only.png': one})
    files = g.list_mask_images(str(tmp_path / 'masks'), 3)
    assert len(files) == 1
    px = g.load_mask_batch(files, [0, 1, 2, 5], 16)
    assert all(np.array_equal(px[i], one) for i in range(4))
    import PIL.Image
    PIL.Image.fromarray(one, 'L').save(tmp_path / 'masks' / 'second.png')
    with pytest.raises(click.UsageError, match='mask_images'):
        g.list_mask_images(str(tmp_path / 'masks'), 3)                 # two masks for three init images
    assert len(g.list_mask_images(str(tmp_path / 'masks'), 2)) == 2
    with pytest.raises(click.UsageError, match='init_images'):
        g.mask_options(None, str(tmp_path / 'masks'), False, 0)
    assert g.mask_options(str(tmp_path / 'init'), None, False, 3) is None
    assert g.mask_options(str(tmp_path / 'init'), str(tmp_path / 'masks'), True, 2) == (g.list_mask_images(str(tmp_path / 'masks'), 2), True)


def test_mask_option_refusals_through_click(tmp_path):
    from click.testing import CliRunner
    import generate_onestep as g
    one = np.full((16, 16), 255, np.uint8)
    _write_images(tmp_path, {'m0.png': one, 'm1.png': one})
    run = lambda *a: CliRunner().invoke(g.main, ['--outdir', str(tmp_path / 'o'), '--repo_id', 'random:tiny', *a])  # noqa: E731
    r = run('--network', 'x.pkl', '--mask_images', str(tmp_path / 'masks'))
    assert r.exit_code == 2 and '--mask_images' in r.output and '--init_images' in r.output
    r = run('--network', 'x.pkl', '--init_images', str(tmp_path / 'init'), '--mask_images', str(tmp_path / 'masks'))
    assert r.exit_code == 2 and '--mask_images' in r.output and 'one per init image' in r.output


def test_composite_takes_kept_pixels_from_the_init_image():
    import generate_onestep as g
    rng = np.random.default_rng(5)
    gen, init = (rng.integers(0, 256, (2, 16, 16, 3), dtype=np.uint8) for _ in range(2))
    mask = rng.integers(0, 256, (2, 16, 16), dtype=np.uint8)
    mask[0, 0, :4] = (0, 127, 128, 255)
    out = g.composite(gen, init, mask)
    keep = mask < 128
    assert out.dtype == np.uint8 and out.shape == gen.shape
    assert np.array_equal(out[keep], init[keep]) and np.array_equal(out[~keep], gen[~keep])
    assert np.array_equal(out[0, 0, 1], init[0, 0, 1]) and np.array_equal(out[0, 0, 2], gen[0, 0, 2])


def test_teacher_image_to_image_needs_an_explicit_strength(tmp_path):
    import click
    from click.testing import CliRunner
    import generate_onestep as g
    _write_images(tmp_path, {})
    d = str(tmp_path / 'init')
    r = CliRunner().invoke(g.main, ['--outdir', str(tmp_path / 'o'), '--repo_id', 'random:tiny', '--network', 'teacher', '--init_images', d])
    assert r.exit_code == 2 and 'teacher' in r.output and '--strength' in r.output
    with pytest.raises(click.UsageError, match='teacher'):
        g.image_to_image_options('teacher', d, None, None, 1, 10)
    files, k, sample = g.image_to_image_options('teacher', d, 0.5, None, 1, 10)
    assert len(files) == 3 and k == 5 and sample is False
    assert g.image_to_image_options('teacher', d, 0.3, True, 1, 10)[1:] == (7, True)
    assert g.image_to_image_options('teacher', d, 0.8, None, 1, None)[1] == 10          # the default --teacher_steps, 50
    with pytest.raises(click.UsageError, match='strength'):
        g.image_to_image_options('teacher', d, 0.05, None, 1, 10)                     # no step would run
    # a snapshot keeps its own rule, and the options without --init_images are refused as before
    assert g.image_to_image_options('x.pkl', d, 0.5, None, 4) == g.init_image_options('x.pkl', d, 0.5, None, 4)
    with pytest.raises(click.UsageError, match='init_images'):
        g.image_to_image_options('teacher', None, 0.5, None, 1, 10)


def test_sampler_argument_checks_need_no_gpu():
    from sid_lsg_amd.sd_util import _teacher_entry, check_mask
    z = torch.zeros(2, 4, 8, 8)
    m = torch.ones(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match='init_latents'):
        check_mask(m, None, z, 'f')
    for bad in (m.float(), m[:, :4], torch.ones(3, 8, 8, dtype=torch.uint8), m[0]):
        with pytest.raises(ValueError, match='mask'):
            check_mask(bad, z, z, 'f')
    assert check_mask(m[:1].bool(), z, z, 'f').shape == (1, 8, 8)
    with pytest.raises(ValueError, match='start_index'):
        _teacher_entry(z, None, 1, None, 4, 'f')
    with pytest.raises(ValueError, match='start_index'):
        _teacher_entry(z, z, 4, None, 4, 'f')
    with pytest.raises(ValueError, match='init_latents'):
        _teacher_entry(z, None, 0, m, 4, 'f')
    assert _teacher_entry(z, None, 0, None, 4, 'f') == (None, None, False)
    assert _teacher_entry(z, z, 0, None, 4, 'f')[2] is True and _teacher_entry(z, z, 1, m, 4, 'f')[2] is True
    assert _teacher_entry(z, z, 0, m, 4, 'f')[2] is False          # a mask at full strength starts from pure noise


def test_masked_renoise_is_bound_from_the_header():
    import ctypes
    from sid_lsg_amd._lib import lib
    want = [ctypes.c_void_p] * 8 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    assert lib.protos['sidlsg_masked_renoise'] == want and lib.protos['sidlsg_masked_renoise_f32'] == want
