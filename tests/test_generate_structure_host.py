"""The structure of the generation path: the named option tuples of generate_onestep.py, its one file lister and one report writer, the
option surface of both command lines (host, no GPU), and the launch sequence of the one teacher loop under sd_util.teacher_sample_i2i /
teacher_sample_solver_i2i (one GPU test).  Expected values are written out: they are what the code before the restructuring returned."""
import json
import math
import os
import re

import click
import numpy as np
import pytest
import torch
from click.testing import CliRunner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def dirs(tmp_path):
    """init/: a.png, b.PNG + a text file + a sub-directory; masks/: m.png; three/: three images."""
    import PIL.Image
    for d, names in (('init', ['b.PNG', 'a.png']), ('masks', ['m.png']), ('three', ['0.png', '1.jpg', '2.jpeg'])):
        (tmp_path / d).mkdir()
        for n in names:
            PIL.Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(tmp_path / d / n))
    (tmp_path / 'init' / 'notes.txt').write_text('not an image')
    (tmp_path / 'init' / 'sub.png').mkdir()
    return tmp_path


def _accepted(g, d):
    """(option function result, expected plain tuple, expected field names), one accepted argument set per group."""
    init, files = str(d / 'init'), [str(d / 'init' / 'a.png'), str(d / 'init' / 'b.PNG')]
    mask = [str(d / 'masks' / 'm.png')]
    return [
        (g.teacher_options('teacher', None, None), (50, 7.5), ('steps', 'guidance_scale')),
        (g.teacher_options('teacher', 4, 2.0), (4, 2.0), ('steps', 'guidance_scale')),
        (g.image_to_image_options('snap.pkl', init, 0.5, True, 4), (files, 2, True), ('files', 'start', 'sample_posterior')),
        (g.image_to_image_options('teacher', init, 0.6, None, 1, 5), (files, 2, False), ('files', 'start', 'sample_posterior')),
        (g.mask_options(init, str(d / 'masks'), True, 2), (mask, True), ('files', 'composite')),
        (g.control_options('random:controlnet', init, None), ('random:controlnet', files, 1.0), ('spec', 'files', 'scale')),
        (g.control_edge_options('random:controlnet', 'canny', None, None, True, None, 64), (True, 100, 200, True, 1),
         ('preprocess', 'low', 'high', 'adherence', 'tolerance')),
        (g.control_edge_options('random:controlnet', None, 50, 60, True, 0, 64), (False, 50, 60, True, 0),
         ('preprocess', 'low', 'high', 'adherence', 'tolerance')),
        (g.ip_options('random:ip-adapter', 'random:clip-tiny', init, 0.5), ('random:ip-adapter', 'random:clip-tiny', files, 0.5),
         ('adapter', 'image_encoder', 'files', 'scale')),
        (g.lora_options(('random:lora', 'random:lora:8'), (0.5,)), (['random:lora', 'random:lora:8'], [0.5, 0.5]), ('specs', 'scales')),
        (g.fidelity_options(init, True, None, None), (None, None), ('lpips_vgg', 'lpips_lin')),
        (g.fidelity_options(init, True, 'random:lpips-vgg:1', 'random:lpips-vgg:1'), ('random:lpips-vgg:1', 'random:lpips-vgg:1'), ('lpips_vgg', 'lpips_lin')),
        (g.diversity_options(True, 2, 'random:lpips-vgg', 'random:lpips-vgg', [3, 0, 1, 2]), ('random:lpips-vgg', 'random:lpips-vgg', {0: [0, 1], 1: [2, 3]}),
         ('lpips_vgg', 'lpips_lin', 'groups')),
    ]


def test_option_results_equal_the_plain_tuples(dirs):
    import generate_onestep as g
    for got, want, _ in _accepted(g, dirs):
        assert tuple(got) == want and got == want and len(got) == len(want)
        assert [got[i] for i in range(len(want))] == list(want)          # indexable and unpackable, as the host tests use them


def test_option_results_are_named_tuples(dirs):
    import generate_onestep as g
    for got, want, fields in _accepted(g, dirs):
        assert isinstance(got, tuple) and type(got) is not tuple and got._fields == fields, (type(got), fields)
        assert tuple(getattr(got, f) for f in fields) == want
    # absent options stay None, and the solver options stay a dict
    assert g.teacher_options('snap.pkl', None, None) is None and g.lora_options((), ()) is None and g.mask_options(None, None, False, 0) is None
    assert g.teacher_solver_options('teacher', teacher_eta=1.0) == dict(solver='ddim', spacing=None, eta=1.0, guidance_rescale=0.0, negative_prompt=None)


def test_refused_options_keep_their_messages(dirs):
    import generate_onestep as g
    init = str(dirs / 'init')
    refused = [
        (lambda: g.teacher_options('snap.pkl', 4, None),
         '--teacher_steps apply to --network teacher only: a distilled generator is sampled without guidance in --num_steps_eval steps'),
        (lambda: g.image_to_image_options('snap.pkl', None, 0.5, None, 1), '--strength apply to --init_images only'),
        (lambda: g.image_to_image_options('teacher', init, None, None, 1, 5),
         '--init_images with --network teacher: image-to-image with the teacher sampler needs an explicit --strength (the share of the '
         '--teacher_steps steps that run)'),
        (lambda: g.mask_options(None, str(dirs / 'masks'), False, 0), '--mask_images applies to --init_images only: the init image is the region that is kept'),
        (lambda: g.control_options(None, init, None), '--control_images needs --controlnet (a ControlNet directory or random:controlnet[:seed])'),
        (lambda: g.control_edge_options(None, 'canny', None, None, False, None, 64), '--control_preprocess apply to --controlnet only'),
        (lambda: g.ip_options(None, None, None, 0.5), '--ip_scale applies to --ip_adapter / --ip_image_encoder / --ip_images only'),
        (lambda: g.lora_options((), (0.5,)), '--lora_scale applies to --lora only'),
        (lambda: g.fidelity_options(None, True, None, None), '--fidelity applies to --init_images only: an output is compared with the init image it started from'),
        (lambda: g.diversity_options(True, 1, 'random:lpips-vgg', 'random:lpips-vgg', [0, 1]),
         '--diversity needs --seeds_per_prompt K with K >= 2: the K samples of one prompt are compared with each other'),
    ]
    for call, message in refused:
        with pytest.raises(click.UsageError) as e:
            call()
        assert e.value.message == message


def test_one_file_lister_under_the_four_names(dirs):
    import generate_onestep as g
    init, three = str(dirs / 'init'), str(dirs / 'three')
    want = [os.path.join(init, 'a.png'), os.path.join(init, 'b.PNG')]          # sorted by name; the text file and the directory are left out
    assert g.list_init_images(init) == g.list_control_images(init) == g.list_ip_images(init) == g.image_files(init, '--any') == want
    # the mask's count rule: one for all, or one per init image
    assert g.list_mask_images(str(dirs / 'masks'), 5) == [os.path.join(str(dirs / 'masks'), 'm.png')]
    assert g.list_mask_images(three, 3) == [os.path.join(three, n) for n in ('0.png', '1.jpg', '2.jpeg')]
    assert g.list_mask_images(init, 2) == want
    with pytest.raises(click.UsageError) as e:
        g.list_mask_images(init, 3)
    assert e.value.message == f'--mask_images {init}: 2 PNG or JPEG files, expected 1 or one per init image (3)'
    (dirs / 'empty').mkdir()
    for lister, flag in ((g.list_init_images, '--init_images'), (g.list_control_images, '--control_images'), (g.list_ip_images, '--ip_images'),
                         (lambda p: g.list_mask_images(p, 2), '--mask_images')):
        with pytest.raises(click.UsageError) as e:
            lister(str(dirs / 'missing'))
        assert e.value.message == f'{flag} {dirs / "missing"}: not a directory'
        with pytest.raises(click.UsageError) as e:
            lister(str(dirs / 'empty'))
        assert e.value.message == (f'{flag} {dirs / "empty"}: 0 PNG or JPEG files, expected 1 or one per init image (2)' if flag == '--mask_images'
                                   else f'{flag} {dirs / "empty"}: no PNG or JPEG files')


def test_one_loader_under_init_and_mask(dirs):
    """Both take the centre crop of the shorter side; RGB + LANCZOS against 'L' + NEAREST; a file of the right size is not resampled."""
    import PIL.Image
    import generate_onestep as g
    a = np.zeros((8, 12, 3), np.uint8)
    a[:, 2:10] = np.arange(8, dtype=np.uint8)[None, :, None] * 30          # the centre 8 x 8 crop is a ramp, the margins are 0
    PIL.Image.fromarray(a).save(str(dirs / 'wide.png'))
    assert (g.load_init_image(str(dirs / 'wide.png'), 8) == a[:, 2:10]).all()
    assert (g.load_mask_image(str(dirs / 'wide.png'), 8) == a[:, 2:10, 0]).all()
    small = g.load_mask_image(str(dirs / 'wide.png'), 4)
    assert small.shape == (4, 4) and small.dtype == np.uint8 and set(np.unique(small)) <= set(np.unique(a))          # NEAREST makes no new value
    assert g.load_init_image(str(dirs / 'wide.png'), 4).shape == (4, 4, 3)
    assert g.load_init_batch([str(dirs / 'wide.png')], [0, 3], 8).shape == (2, 8, 8, 3) and g.load_mask_batch([str(dirs / 'wide.png')], [5], 8).shape == (1, 8, 8)


def test_write_report_world_size_one(tmp_path):
    import generate_onestep as g
    seen = []

    def aggregate(rows):
        seen.append(list(rows))
        return dict(psnr=float('inf'), lpips=float('nan'), n=len(rows))
    path = str(tmp_path / 'new' / 'fidelity.json')          # the directory is made
    rows = {'000002.png': dict(psnr=float('inf')), '000000.png': dict(psnr=31.5), '000001.png': dict(psnr=float('nan'))}
    report = g.write_report(rows, path, dict(network='teacher', strength=None), 'per_image', aggregate)
    assert list(report) == ['options', 'per_image', 'mean'] and list(report['per_image']) == ['000000.png', '000001.png', '000002.png']
    assert seen == [['000000.png', '000001.png', '000002.png']]          # the aggregate sees the sorted rows
    text = open(path).read()
    assert text.startswith('{\n "options": {\n  "network": "teacher",\n  "strength": null\n },\n "per_image": {\n  "000000.png": {\n   "psnr": 31.5')       # indent 1
    back = json.loads(text, object_pairs_hook=lambda pairs: pairs)
    assert [k for k, _ in back] == ['options', 'per_image', 'mean']
    back = json.loads(text)
    assert back['options'] == dict(network='teacher', strength=None) and back['per_image']['000000.png'] == dict(psnr=31.5)
    assert math.isinf(back['per_image']['000002.png']['psnr']) and math.isnan(back['per_image']['000001.png']['psnr'])
    assert math.isinf(back['mean']['psnr']) and math.isnan(back['mean']['lpips']) and back['mean']['n'] == 3
    # diversity's rows: integer group keys, sorted as numbers, written as strings
    report = g.write_report({10: dict(v=1.0), 2: dict(v=2.0), 0: dict(v=3.0)}, str(tmp_path / 'diversity.json'), {}, 'per_prompt', lambda rows: dict(n=len(rows)))
    assert list(report) == ['options', 'per_prompt', 'mean'] and list(report['per_prompt']) == ['0', '2', '10']
    assert list(json.load(open(str(tmp_path / 'diversity.json')))['per_prompt']) == ['0', '2', '10']


ONESTEP_OPTIONS = ['--network', '--outdir', '--seeds', '--subdirs', '--batch', '--num', '--init_timestep', '--text_prompts', '--repo_id', '--resolution',
                   '--use_fp16', '--enable_compress_npz', '--num_steps_eval', '--custom_seed', '--teacher_steps', '--guidance_scale', '--teacher_sampler',
                   '--teacher_spacing', '--teacher_eta', '--guidance_rescale', '--negative_prompt', '--init_images', '--strength', '--sample_posterior',
                   '--mask_images', '--mask_composite', '--controlnet', '--control_images', '--control_scale', '--control_preprocess', '--canny_low',
                   '--canny_high', '--control_adherence', '--edge_tolerance', '--ip_adapter', '--ip_image_encoder', '--ip_images', '--ip_scale', '--lora',
                   '--lora_scale', '--fidelity', '--lpips_vgg', '--lpips_lin', '--seeds_per_prompt', '--diversity', '--text_encoder', '--help']
HPSV2_OPTIONS = ['--network', '--outdir', '--seeds', '--subdirs', '--batch', '--num', '--init_timestep', '--repo_id', '--resolution', '--num_steps_eval',
                 '--text_encoder', '--teacher_steps', '--guidance_scale', '--hps_prompts', '--hps_checkpoint', '--hps_tokenizer', '--hps_arch', '--score_only',
                 '--help']


def test_help_lists_the_same_options_in_the_same_order():
    import generate_hpsv2
    import generate_onestep
    for main, want in ((generate_onestep.main, ONESTEP_OPTIONS), (generate_hpsv2.main, HPSV2_OPTIONS)):
        res = CliRunner().invoke(main, ['--help'])
        assert res.exit_code == 0, res.output
        assert re.findall(r'^  (--[a-z_0-9]+)', res.output, re.M) == want


def test_no_index_on_an_option_object_remains():
    """main() and its helpers read the option tuples by field name: no `teacher[1]`, `edge_opt[3]` ... in either script."""
    names = r'(?:teacher|img2img|masks?|control|edge(?:_opt)?|ip|fid|div|lora(?:_opt)?|o\.\w+)'
    for script in ('generate_onestep.py', 'generate_hpsv2.py'):
        src = open(os.path.join(ROOT, script)).read()
        assert re.findall(rf'\b{names}\[\d\]', src) == [], script


# ------------------------------------------------------------------------------------------------
# The launch sequence of the teacher loop, 3 steps, as read from the two loops it replaced.  Entries: ('noisy_input', init latents given),
# ('unet',), ('ddim_step', last), ('cfg_rescale_stats',), ('randn',), ('masked_renoise', want_input) and
# ('solver_step', last, x0p: None or 'prev' = the x0 the step before returned, noise given, scale given, need_prev, which of the two x0 buffers).
U = ('unet',)


def S(last, x0p, noise, scale, need_prev, buf):
    return ('solver_step', last, x0p, noise, scale, need_prev, buf)


DDIM_SEQUENCES = {
    'plain': [('noisy_input', False), U, ('ddim_step', False), U, ('ddim_step', False), U, ('ddim_step', True)],
    'init_start_1': [('noisy_input', True), U, ('ddim_step', False), U, ('ddim_step', True)],
    # a mask at start_index 0: pure-noise start, last=True on every step, the final masked_renoise(want_input=False)
    'mask_start_0': [('noisy_input', False), U, ('ddim_step', True), ('masked_renoise', True), U, ('ddim_step', True), ('masked_renoise', True),
                     U, ('ddim_step', True), ('masked_renoise', False)],
}
SOLVER_SEQUENCES = {      # DPM-Solver++ 2M: first order at its first executed step, the x0 row at the last; c_prev of steps 1 .. N-2 only
    'plain': [('noisy_input', False), U, S(False, None, False, False, False, 0), U, S(False, 'prev', False, False, True, 1),
              U, S(True, None, False, False, False, 0)],
    'init_start_1': [('noisy_input', True), U, S(False, None, False, False, False, 0), U, S(True, None, False, False, False, 1)],
    'mask_start_0': [('noisy_input', False), U, S(True, None, False, False, False, 0), ('masked_renoise', True),
                     U, S(True, 'prev', False, False, True, 1), ('masked_renoise', True), U, S(True, None, False, False, False, 0), ('masked_renoise', False)],
    # DDIM with eta = 1 (c_n non-zero at every step of the SD schedule) and guidance rescale: one statistics launch and one draw per step
    'eta_1_rescale': [('noisy_input', False)] + [e for i in range(3) for e in (U, ('cfg_rescale_stats',), ('randn',), S(i == 2, None, True, True, False, i & 1))],
}


@pytest.mark.gpu
def test_teacher_loop_call_sequences(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd import ops, sd_util
    dev = torch.device('cuda:0')
    unet, vae, sched, te, tok = sd_util.load_sd15('random:tiny', 'random:tiny', dev, torch.bfloat16)
    gen = torch.Generator().manual_seed(5)
    z, z0 = (torch.randn(2, 4, 8, 8, generator=gen).to(dev) for _ in range(2))
    mask = torch.zeros(1, 8, 8, dtype=torch.uint8, device=dev)
    mask[:, :, 3:] = 1
    calls, state = [], dict(bufs=[], x0=None)

    def record(name, entry):
        real = getattr(ops, name)

        def wrapper(*a, **kw):
            calls.append(entry(*a, **kw))
            return real(*a, **kw)
        monkeypatch.setattr(ops, name, wrapper)
    record('noisy_input', lambda x0, *a, **kw: ('noisy_input', x0 is not None))
    record('ddim_step', lambda *a, last=False, **kw: ('ddim_step', last))
    record('cfg_rescale_stats', lambda *a, **kw: ('cfg_rescale_stats',))
    record('masked_renoise', lambda *a, want_input=True, **kw: ('masked_renoise', want_input))
    real_solver_step, real_forward = ops.solver_step, unet.forward_nhwc

    def solver_step(*a, x0p=None, noise=None, scale=None, last=False, x0_out=None, need_prev=None, **kw):
        if x0_out.data_ptr() not in state['bufs']:
            state['bufs'].append(x0_out.data_ptr())
        calls.append(S(last, None if x0p is None else 'prev' if x0p is state['x0'] else 'other', noise is not None, scale is not None, need_prev,
                       state['bufs'].index(x0_out.data_ptr())))
        out = real_solver_step(*a, x0p=x0p, noise=noise, scale=scale, last=last, x0_out=x0_out, need_prev=need_prev, **kw)
        state['x0'] = out[2]
        return out
    monkeypatch.setattr(ops, 'solver_step', solver_step)
    monkeypatch.setattr(unet, 'forward_nhwc', lambda *a, **kw: calls.append(U) or real_forward(*a, **kw))

    def randn(shape):
        calls.append(('randn',))
        return torch.randn(shape, device=dev, dtype=torch.float32)
    common = dict(unet=unet, latents=z, contexts=['a photo', 'a drawing'], noise_scheduler=sched, text_encoder=te, tokenizer=tok, resolution=64,
                  guidance_scale=2.0, num_inference_steps=3)
    conditions = dict(plain={}, init_start_1=dict(init_latents=z0, start_index=1), mask_start_0=dict(init_latents=z0, start_index=0, mask=mask),
                      eta_1_rescale=dict(solver='ddim', eta=1.0, guidance_rescale=0.7))
    for fn, sequences in ((sd_util.teacher_sample_i2i, DDIM_SEQUENCES), (sd_util.teacher_sample_solver_i2i, SOLVER_SEQUENCES)):
        for case, want in sequences.items():
            calls.clear()
            state.update(bufs=[], x0=None)
            before = dict(ops.solver_launches)
            kw = dict(conditions[case], randn=randn) if fn is sd_util.teacher_sample_solver_i2i else conditions[case]
            out = fn(**common, **kw)
            assert calls == want, (fn.__name__, case, calls)
            assert out.shape == z.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
            got = {k: ops.solver_launches[k] - before[k] for k in before}
            assert got == {k: sum(1 for c in want if c[0] == k) for k in before}, (fn.__name__, case, got)
    # return_images goes through decode_latents: the images sid_sd_sampler's tail gives for the same latent
    lat = sd_util.teacher_sample_i2i(**common)
    img = sd_util.teacher_sample_i2i(**common, return_images=True, vae=vae)
    assert img.shape == (2, 3, 64, 64) and torch.equal(img, sd_util.decode_latents(vae, lat))
