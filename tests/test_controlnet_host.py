"""ControlNet, host side (no GPU): parameter names and shapes against the torch.nn restatement, every refusal of a config / a weights
file / the command line, the control-image file rule, the MAC count of tools/controlnet_cost.py, and the precondition of the GPU tests
(tests/test_gpu_controlnet.py): with the seeded weights used there the ControlNet changes the REFERENCE's output by well over 10 %."""
import json
import os

import numpy as np
import pytest
import torch

import controlnet_ref as cr

SD15_CONFIG = dict(block_out_channels=[320, 640, 1280, 1280], cross_attention_dim=768, attention_head_dim=8, use_linear_projection=False,
                   layers_per_block=2, norm_num_groups=32, conditioning_embedding_out_channels=[16, 32, 96, 256], conditioning_channels=3,
                   global_pool_conditions=False, class_embed_type=None, addition_embed_type=None)


def _shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


@pytest.mark.parametrize('name', ['tiny', 'tiny21', 'sd15', 'sd21-base'])
def test_state_dict_names_and_shapes_match_the_reference(name):
    from oracle.unet_ref import CONFIGS as RC
    from sid_lsg_amd.controlnet import HipControlNet
    from sid_lsg_amd.unet import CONFIGS
    with torch.device('meta'):
        ref = cr.ControlNetRef(RC[name])
    got, want = _shapes(HipControlNet(CONFIGS[name])), _shapes(ref)          # HipControlNet builds on the meta device by itself
    assert list(got) and set(got) == set(want), sorted(set(got) ^ set(want))[:8]
    assert got == want, [(k, got[k], want[k]) for k in got if got[k] != want[k]][:8]
    assert got['controlnet_down_blocks.11.weight'] == (want['mid_block.resnets.0.conv1.weight'][0],) * 2 + (1, 1)
    assert sum(k.startswith('controlnet_down_blocks.') for k in got) == 24 and 'controlnet_mid_block.bias' in got
    if name == 'sd15':
        assert got['controlnet_cond_embedding.conv_in.weight'] == (16, 3, 3, 3) and got['controlnet_cond_embedding.blocks.5.weight'] == (256, 96, 3, 3)
        assert got['controlnet_cond_embedding.conv_out.weight'] == (320, 256, 3, 3)


@pytest.mark.parametrize('key,value', [('global_pool_conditions', True), ('class_embed_type', 'timestep'), ('addition_embed_type', 'text'),
                                       ('conditioning_channels', 1), ('block_out_channels', [320, 640, 1280]), ('cross_attention_dim', 1024),
                                       ('use_linear_projection', True), ('attention_head_dim', [5, 10, 20, 20]), ('layers_per_block', 1),
                                       ('conditioning_embedding_out_channels', [16, 32, 100, 256])])
def test_config_refusals_name_the_key(key, value):
    from sid_lsg_amd.controlnet import check_controlnet_config
    from sid_lsg_amd.unet import CONFIGS
    assert check_controlnet_config(dict(SD15_CONFIG), CONFIGS['sd15']) == (16, 32, 96, 256)
    with pytest.raises(ValueError, match=key):
        check_controlnet_config(dict(SD15_CONFIG, **{key: value}), CONFIGS['sd15'])


def test_architecture_mismatch_names_the_field():
    from sid_lsg_amd.controlnet import check_same_architecture
    from sid_lsg_amd.unet import CONFIGS
    check_same_architecture(CONFIGS['sd15'], CONFIGS['sd15'])
    with pytest.raises(ValueError, match='cross_attention_dim'):
        check_same_architecture(CONFIGS['sd21-base'], CONFIGS['sd15'])
    with pytest.raises(ValueError, match='block_out_channels'):
        check_same_architecture(CONFIGS['tiny'], CONFIGS['tiny21'])


def _tiny_dir(tmp_path, mutate=None, config=None):
    from safetensors.torch import save_file
    _, _, _, csd = cr.make_pair('tiny')
    sd = {k: v.contiguous() for k, v in csd.items()}
    if mutate:
        mutate(sd)
    d = tmp_path / 'cn'
    d.mkdir()
    save_file(sd, str(d / 'diffusion_pytorch_model.safetensors'))
    cfg = dict(block_out_channels=[32, 64, 128, 128], cross_attention_dim=64, attention_head_dim=[2, 2, 4, 4], use_linear_projection=False,
               layers_per_block=2, norm_num_groups=8, conditioning_embedding_out_channels=list(cr.TINY_COND_CHANNELS))
    cfg.update(config or {})
    (d / 'config.json').write_text(json.dumps(cfg))
    return str(d)


def test_directory_refusals_name_the_key(tmp_path):
    """The directory form is checked before anything touches a GPU: the config against the UNet, then every key and shape."""
    from sid_lsg_amd.sd_util import load_controlnet
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    unet = HipUNet2DCondition(CONFIGS['tiny'])
    (tmp_path / 'a').mkdir(), (tmp_path / 'b').mkdir(), (tmp_path / 'c').mkdir(), (tmp_path / 'd').mkdir()
    with pytest.raises(ValueError, match='missing key controlnet_mid_block.weight'):
        load_controlnet(_tiny_dir(tmp_path / 'a', lambda sd: sd.pop('controlnet_mid_block.weight')), unet, 'cpu')
    with pytest.raises(ValueError, match=r'controlnet_down_blocks\.3\.weight has shape \(32, 32\)'):
        load_controlnet(_tiny_dir(tmp_path / 'b', lambda sd: sd.update({'controlnet_down_blocks.3.weight': torch.zeros(32, 32)})), unet, 'cpu')
    with pytest.raises(ValueError, match='cross_attention_dim'):
        load_controlnet(_tiny_dir(tmp_path / 'c', config=dict(cross_attention_dim=96)), unet, 'cpu')
    with pytest.raises(ValueError, match='unexpected key up_blocks.0.foo'):
        load_controlnet(_tiny_dir(tmp_path / 'd', lambda sd: sd.update({'up_blocks.0.foo': torch.zeros(1)})), unet, 'cpu')
    with pytest.raises(FileNotFoundError):
        load_controlnet(str(tmp_path / 'nowhere'), unet, 'cpu')
    with pytest.raises(TypeError):
        load_controlnet('random:controlnet', torch.nn.Linear(2, 2), 'cpu')


def test_random_spec_parsing():
    from sid_lsg_amd.controlnet import parse_random_spec
    assert parse_random_spec('random:controlnet') is None
    assert parse_random_spec('random:controlnet:0') == 0 and parse_random_spec('RANDOM:ControlNet:17') == 17
    for bad in ('random:controlnet:x', 'random:controlnet:-1', 'random:controlnet:1:2', 'random:tiny', 'random:controlnets'):
        with pytest.raises(ValueError):
            parse_random_spec(bad)


def test_prepare_refuses_bad_arguments_before_any_launch():
    from sid_lsg_amd.controlnet import HipControlNet
    from sid_lsg_amd.unet import CONFIGS
    net = HipControlNet(CONFIGS['tiny'])
    with pytest.raises(RuntimeError, match='not materialised'):
        net.prepare(torch.zeros(1, 64, 64, 3, dtype=torch.uint8))
    net._flat = {}           # the argument checks below come before the first use of the buffers
    for img, kw, msg in ((torch.zeros(1, 3, 64, 64, dtype=torch.uint8), {}, 'uint8'), (torch.zeros(1, 64, 64, 3), {}, 'uint8'),
                         (torch.zeros(1, 60, 64, 3, dtype=torch.uint8), {}, 'multiples of 8'),
                         (torch.zeros(1, 64, 64, 3, dtype=torch.uint8), dict(scale=-0.5), 'scale'),
                         (torch.zeros(1, 64, 64, 3, dtype=torch.uint8), dict(dup=3), 'dup')):
        with pytest.raises(ValueError, match=msg):
            net.prepare(img, **kw)
    with pytest.raises(ValueError, match='gradient'):
        net.materialize('cpu', with_grad_buffers=True)
    with pytest.raises(ValueError, match='cond_channels'):
        HipControlNet(CONFIGS['tiny'], cond_channels=(8, 16, 20, 32))


def _write_png(path, w, h, value):
    import PIL.Image
    PIL.Image.fromarray(np.full((h, w, 3), value, dtype=np.uint8)).save(path)


def test_control_image_file_rule_and_size_refusal(tmp_path):
    import click
    import generate_onestep as g
    d = tmp_path / 'ctl'
    d.mkdir()
    _write_png(str(d / 'b.png'), 16, 16, 20)
    _write_png(str(d / 'a.png'), 16, 16, 10)
    (d / 'notes.txt').write_text('not an image')
    files = g.list_control_images(str(d))
    assert [os.path.basename(f) for f in files] == ['a.png', 'b.png']
    batch = g.load_control_batch(files, [0, 1, 2, 5], 16)
    assert batch.shape == (4, 16, 16, 3) and batch.dtype == np.uint8
    assert batch[:, 0, 0, 0].tolist() == [10, 20, 10, 20]                     # sample idx -> file idx mod len(files)
    _write_png(str(d / 'c.png'), 24, 16, 30)
    with pytest.raises(click.UsageError) as ei:
        g.load_control_batch(g.list_control_images(str(d)), [2], 16)
    assert 'c.png' in str(ei.value) and '24 x 16' in str(ei.value) and '16 x 16' in str(ei.value)
    with pytest.raises(click.UsageError):
        g.list_control_images(str(tmp_path / 'missing'))
    (tmp_path / 'empty').mkdir()
    with pytest.raises(click.UsageError):
        g.list_control_images(str(tmp_path / 'empty'))


def test_cli_usage_errors(tmp_path):
    from click.testing import CliRunner
    import generate_onestep as g
    d = tmp_path / 'ctl'
    d.mkdir()
    _write_png(str(d / 'a.png'), 16, 16, 10)
    base = ['--network', 'teacher', '--outdir', str(tmp_path / 'out'), '--repo_id', 'random:tiny']
    for extra, msg in ((['--controlnet', 'random:controlnet'], '--controlnet needs --control_images'),
                       (['--control_images', str(d)], '--control_images needs --controlnet'),
                       (['--control_scale', '0.5'], '--control_scale applies to'),
                       (['--controlnet', 'random:controlnet', '--control_images', str(d), '--control_scale', '-1'], 'control_scale'),
                       (['--controlnet', 'random:controlnet', '--control_images', str(tmp_path / 'none')], 'not a directory')):
        res = CliRunner().invoke(g.main, base + extra)
        assert res.exit_code == 2 and msg in res.output, (extra, res.output)
    assert g.control_options(None, None, None) is None
    spec, files, scale = g.control_options('random:controlnet:3', str(d), None)
    assert (spec, len(files), scale) == ('random:controlnet:3', 1, 1.0)
    assert g.control_options('x', str(d), 0.0)[2] == 0.0


def _count_macs(module, run):
    """Multiply-accumulates of `run()` by forward hooks on the contractions of a reference module (batch of one): Conv2d, Linear and the
    two matrix products of every Attention."""
    from oracle.unet_ref import Attention
    total = [0]

    def conv(m, inp, out):
        total[0] += out.shape[2] * out.shape[3] * m.out_channels * m.in_channels * m.kernel_size[0] * m.kernel_size[1]

    def linear(m, inp, out):
        total[0] += out.numel() // m.out_features * m.out_features * m.in_features

    def attn(m, inp, out):
        x = inp[0]
        nk = x.shape[1] if len(inp) < 2 or inp[1] is None else inp[1].shape[1]
        total[0] += 2 * x.shape[1] * nk * x.shape[2]
    hooks = []
    for m in module.modules():
        fn = conv if isinstance(m, torch.nn.Conv2d) else linear if isinstance(m, torch.nn.Linear) else attn if isinstance(m, Attention) else None
        if fn is not None:
            hooks.append(m.register_forward_hook(fn))
    run()
    for h in hooks:
        h.remove()
    return total[0]


@pytest.mark.parametrize('name,h,w', [('tiny', 8, 16), ('tiny21', 16, 8)])
def test_mac_count_matches_hooks_on_the_reference(name, h, w):
    from oracle.unet_ref import CONFIGS as RC
    from sid_lsg_amd.controlnet import controlnet_forward_macs
    from sid_lsg_amd.unet import CONFIGS
    cfg = RC[name]
    ref = cr.ControlNetRef(cfg).eval()
    x, t, ctx = torch.zeros(1, 4, h, w), torch.tensor([10]), torch.zeros(1, cfg.text_len, cfg.cross_attention_dim)
    cond = torch.zeros(1, 3, 8 * h, 8 * w)
    with torch.no_grad():
        prep = _count_macs(ref.controlnet_cond_embedding, lambda: ref.embed(cond))
        both = _count_macs(ref, lambda: ref(x, t, ctx, cond))
    step, prepare = controlnet_forward_macs(CONFIGS[name], h, w)
    assert prepare == prep and step == both - prep


def test_cost_tool_predicted_ratio():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'controlnet_cost.py')
    spec = importlib.util.spec_from_file_location('controlnet_cost', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from sid_lsg_amd.controlnet import controlnet_forward_macs
    from sid_lsg_amd.unet import CONFIGS, unet_forward_macs
    u = unet_forward_macs(CONFIGS['sd15'], 64, 64)
    c, _ = controlnet_forward_macs(CONFIGS['sd15'], 64, 64)
    assert mod.predicted_ratio('sd15', 64, 64) == (u + c) / u and 1.2 < (u + c) / u < 1.5


@pytest.mark.parametrize('name', ['tiny', 'tiny21'])
def test_seeded_controlnet_changes_the_reference_output(name):
    """Precondition of every tolerance test on the GPU, asserted on the reference alone (fp64, CPU): with the seeded weights and inputs of
    tests/test_gpu_controlnet.py, |out_control - out_plain| / |out_plain| >= 0.1 at scale 1, so an implementation that ignores the
    control state cannot pass them."""
    unet, cnet, _, _ = cr.make_pair(name)
    x, t, ctx, img = cr.make_inputs(name, w=16)
    plain, ctl = cr.ref_outputs(unet, cnet, x, t, ctx, img, 1.0)
    rel = ((ctl - plain).norm() / plain.norm()).item()
    print(f'{name}: control effect on the reference {rel:.3f}')
    assert rel >= 0.1
    # and the controlled reference with zero residuals is the plain one
    zeros = [torch.zeros(1, dtype=plain.dtype)] * 12
    again = unet(x.to(plain.dtype), t, encoder_hidden_states=ctx.to(plain.dtype), down_residuals=zeros, mid_residual=zeros[0]).sample
    assert torch.equal(again, plain)
