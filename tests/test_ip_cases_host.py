"""CPU checks behind tests/test_gpu_ip_adapter.py: the needle inputs of tests/ip_cases.py tell a right two-set attention from a wrong
one at the bound the GPU test uses, the adapter's loader (key table, refusals, file round trips), the command-line option rules, and the
precondition that the seeded adapter changes the reference UNet's output by more than 10 %."""
import os

import click
import pytest
import torch

import ip_adapter_ref as ir
import ip_cases as ic

F32, F64 = torch.float32, torch.float64


# ---- the inputs discriminate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', ic.HOST_SCALES)
@pytest.mark.parametrize('c', ic.HOST_CASES, ids=ic.case_id)
def test_emulation_is_inside_the_bound_and_every_mutation_misses_it_tenfold(c, s):
    """FWD_TOL = 1.2e-2 per (batch, head) slice.  Measured over all cases: the emulation at most 0.36 of the bound; the weakest mutation
    is 'double' (17 x the bound on the image set, 20 x on the text set), 'zero_row' on the text set 15.7 x, every other one >= 63 x."""
    for kind in ic.KINDS + ('biased',):
        x, ref = ic.case_inputs(c, kind), ic.case_ref(c, kind, s)
        e = ic.close_slices(ic.cross2_emulated(x, s, c.H), ref, ic.FWD_TOL, c.H, f'{ic.case_id(c)} {kind} emulation')
        assert e > 0
        targets = ('image', 'text') if kind == 'biased' else (kind,)
        for target in targets:
            for m in ic.mutations_for(c, s, target, kind):
                r = ic.slice_rel_err(ic.cross2_ref64(x, s, c.H, m, target), ref, c.H)
                assert r > 10 * ic.FWD_TOL, f'{ic.case_id(c)} s={s} {kind}: mutation {m} of the {target} set is only {r / ic.FWD_TOL:.1f} x the bound'


def test_every_mutation_is_exercised():
    seen = {(t, m) for c in ic.HOST_CASES for s in ic.HOST_SCALES for t in ic.KINDS for m in ic.mutations_for(c, s, t, t)}
    assert seen == {('image', m) for m in ic.SET_MUTATIONS + ic.IMAGE_ONLY_MUTATIONS} | {('text', m) for m in ic.SET_MUTATIONS}
    assert ic.mutations_for(ic.HOST_CASES[0], 1.0, 'image', 'biased') == ('zero_row',)


def test_needle_positions_and_pre_scaled_twin():
    c = ic.Case2(2, 4, 130, 77, 17, 40, False)
    x = ic.case_inputs(c, 'image')
    assert x['pos2'][0, 0] == 16 and x['pos'][0, 0] == 76 and len(set(x['pos2'].flatten().tolist())) > 3
    xp = ic.make_inputs(c._replace(ps=True), 'image')
    # the pre-scaled twin (its own seed): the kernel gets q D^-1/2 log2 e, the reference the queries that rounding stands for
    cs = 40 ** -0.5 * ic.LOG2E
    assert torch.equal((xp['q_ref'] * cs).float().to(ic.BF16), xp['q']) and torch.equal(x['q_ref'], x['q'].double())
    # s = 0 is the text set alone
    assert torch.equal(ic.one_set_ref64(x, 4), ic.cross2_ref64(x, 0.0, 4, 'other_row', 'image'))


# ---- loader -----------------------------------------------------------------------------------------------------------------------------
def _cfg(name='sd15'):
    from sid_lsg_amd.unet import CONFIGS
    return CONFIGS[name]


def test_layer_table_is_down_up_mid():
    from sid_lsg_amd import ip_adapter as ipa
    t = ipa.layer_table(_cfg())
    assert [n for n, _, _ in t] == list(range(1, 32, 2))
    assert [c for _, _, c in t] == [320, 320, 640, 640, 1280, 1280] + [1280] * 3 + [640] * 3 + [320] * 3 + [1280]
    assert t[0][1] == 'down_blocks.0.attentions.0' and t[6][1] == 'up_blocks.1.attentions.0' and t[-1][1:] == ('mid_block.attentions.0', 1280)
    keys = ipa.expected_keys(_cfg())
    assert keys[:4] == list(ipa.PROJ_KEYS) and keys[4] == 'ip_adapter.1.to_k_ip.weight' and keys[-1] == 'ip_adapter.31.to_v_ip.weight'
    assert len(keys) == 36


def test_layer_table_matches_the_module_tree():
    from sid_lsg_amd import ip_adapter as ipa
    from sid_lsg_amd.unet import HipUNet2DCondition
    for name in ('tiny', 'tiny40', 'tiny21'):
        net = HipUNet2DCondition(_cfg(name))
        names = {id(m): n for n, m in net.named_modules()}
        layers = net.cross_attention_layers()
        table = ipa.layer_table(_cfg(name))
        assert len(layers) == len(table) == 16
        for m, (_, where, c) in zip(layers, table):
            assert names[id(m)] == where + '.transformer_blocks.0.attn2' and m.to_q.weight.shape[0] == c and m.is_cross


def test_loader_refusals_name_the_problem():
    from sid_lsg_amd import ip_adapter as ipa
    cfg = _cfg('tiny40')
    sd = ipa.random_state_dict(cfg, 32, seed=1)
    assert ipa.check_state_dict(sd, cfg, 32) == 4
    assert all(float(v.abs().max()) > 0 for v in sd.values())

    def bad(change, match, embed=32, exc=ValueError):
        d = dict(sd)
        change(d)
        with pytest.raises(exc, match=match):
            ipa.check_state_dict(d, cfg, embed, where='file.bin')

    bad(lambda d: d.pop('ip_adapter.5.to_v_ip.weight'), 'file.bin: missing key ip_adapter.5.to_v_ip.weight')
    bad(lambda d: d.pop('image_proj.norm.bias'), 'missing key image_proj.norm.bias')
    bad(lambda d: d.update({'ip_adapter.33.to_k_ip.weight': d['ip_adapter.31.to_k_ip.weight']}), 'unexpected key ip_adapter.33.to_k_ip.weight')
    bad(lambda d: d.update({'image_proj.latents': torch.zeros(1, 16, 96)}), 'image_proj.latents.*not supported')
    bad(lambda d: d.update({'image_proj.layers.0.0.to_q.weight': torch.zeros(4, 4)}), 'not supported')
    bad(lambda d: d.update({'ip_adapter.3.to_k_ip.weight': torch.zeros(80, 64)}), r'ip_adapter.3.to_k_ip.weight has shape \(80, 64\), expected \(80, 96\)')
    bad(lambda d: d.update({'image_proj.proj.weight': torch.zeros(33 * 96, 32), 'image_proj.proj.bias': torch.zeros(33 * 96)}), 'T = 33')
    bad(lambda d: d.update({'image_proj.proj.weight': torch.zeros(4 * 96 + 1, 32)}), r'expected \[T \* 96, E\]')
    bad(lambda d: None, 'E = 32, the image encoder has projection_dim 768', embed=768)
    bad(lambda d: d.update({'image_proj.proj.bias': torch.zeros(5 * 96)}), 'image_proj.proj.bias has shape')

    # the other plausible numbering (mid block before the up blocks) is refused by its shapes, not guessed
    t = ipa.layer_table(cfg)
    other = [r for r in t if r[1].startswith('down')] + [t[-1]] + [r for r in t if r[1].startswith('up')]
    swapped = {k: v for k, v in sd.items() if k.startswith('image_proj.')}
    for i, (_, _, c) in enumerate(other):
        for p in 'kv':
            swapped[f'ip_adapter.{2 * i + 1}.to_{p}_ip.weight'] = torch.zeros(c, 96)
    with pytest.raises(ValueError, match=r'ip_adapter.19.to_k_ip.weight has shape \(320, 96\), expected \(160, 96\).*another order is refused'):
        ipa.check_state_dict(swapped, cfg, 32)
    with pytest.raises(ValueError, match='cross_attention_dim|expected'):
        ipa.check_state_dict(sd, _cfg('tiny21'), 32)


def test_file_round_trips_and_inferred_token_count(tmp_path):
    from safetensors.torch import save_file
    from sid_lsg_amd import ip_adapter as ipa
    cfg = _cfg('tiny40')
    sd = ipa.random_state_dict(cfg, 32, seed=5, tokens=7)
    st, bn = str(tmp_path / 'ip.safetensors'), str(tmp_path / 'ip.bin')
    save_file(sd, st)
    torch.save(ipa.nested_state(sd), bn)
    nested = torch.load(bn, weights_only=True)
    assert set(nested) == {'image_proj', 'ip_adapter'} and '1.to_k_ip.weight' in nested['ip_adapter'] and 'proj.weight' in nested['image_proj']
    for path in (st, bn):
        got = ipa.read_state_file(path)
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
        ad = ipa.HipIPAdapter(cfg, got, 'cpu', F32, 32, where=path)
        assert ad.tokens == 7 and ad.embed_dim == 32 and ad.width == sum(2 * c for _, _, c in ipa.layer_table(cfg)) == ad.w_kv.shape[0]
        assert all(torch.equal(v, sd[k]) for k, v in ad.state_dict().items())
        off, c = ad.offsets[3], ad.channels[3]
        assert torch.equal(ad.w_kv[off:off + c], sd['ip_adapter.7.to_k_ip.weight']) and torch.equal(ad.w_kv[off + c:off + 2 * c], sd['ip_adapter.7.to_v_ip.weight'])
    with pytest.raises(FileNotFoundError, match='random:ip-adapter'):
        ipa.read_state_file(str(tmp_path / 'missing.safetensors'))
    other = tmp_path / 'ip.pt'
    other.write_bytes(b'x')
    with pytest.raises(ValueError, match='.safetensors or .bin'):
        ipa.read_state_file(str(other))
    a, b = ipa.random_state_dict(cfg, 32, seed=5), ipa.random_state_dict(cfg, 32, seed=6)
    assert ipa.check_state_dict(a, cfg, 32) == ipa.RANDOM_TOKENS == 4
    assert not torch.equal(a['ip_adapter.1.to_k_ip.weight'], b['ip_adapter.1.to_k_ip.weight'])


def test_random_spec_parsing():
    from sid_lsg_amd import ip_adapter as ipa
    assert ipa.parse_random_spec('random:ip-adapter') is None
    assert ipa.parse_random_spec('random:IP-Adapter:17') == 17
    for bad in ('random:ip-adapter:x', 'random:ip-adapter:1:2', 'random:controlnet', 'random:ip_adapter', 'random:ip-adapter:-1'):
        with pytest.raises(ValueError):
            ipa.parse_random_spec(bad)


def test_clip_vision_config_forms():
    from sid_lsg_amd import clip
    full = clip.CLIP_ARCHS['tiny']
    v = clip.parse_vision_config(full, 'x')
    flat = dict(full['vision_config'], projection_dim=full['projection_dim'], model_type='clip_vision_model')
    f = clip.parse_vision_config(flat, 'x')
    assert vars(v) == vars(f) and v.projection_dim == 32
    with pytest.raises(KeyError, match='projection_dim'):
        clip.parse_vision_config(dict(full['vision_config']), 'x')
    with pytest.raises(KeyError, match='config.patch_size'):
        clip.parse_vision_config({k: v for k, v in flat.items() if k != 'patch_size'}, 'x')
    with pytest.raises(ValueError, match='random:clip-'):
        clip.load_clip_vision('random:vit', 'cpu')
    with pytest.raises(FileNotFoundError, match='config.json'):
        clip.load_clip_vision('/nonexistent/clip', 'cpu')


# ---- command line -----------------------------------------------------------------------------------------------------------------------
def test_ip_option_rules(tmp_path):
    import PIL.Image
    import generate_onestep as go
    assert go.ip_options(None, None, None, None) is None
    with pytest.raises(click.UsageError, match='--ip_scale applies to'):
        go.ip_options(None, None, None, 0.5)
    d = tmp_path / 'imgs'
    d.mkdir()
    for given in (('a.bin', None, None), (None, 'random:clip-tiny', None), (None, None, str(d)), ('a.bin', 'random:clip-tiny', None),
                  ('a.bin', None, str(d)), (None, 'random:clip-tiny', str(d))):
        with pytest.raises(click.UsageError, match='need'):
            go.ip_options(*given, None)
    with pytest.raises(click.UsageError, match='no PNG or JPEG'):
        go.ip_options('a.bin', 'random:clip-tiny', str(d), None)
    with pytest.raises(click.UsageError, match='not a directory'):
        go.ip_options('a.bin', 'random:clip-tiny', str(d / 'none'), None)
    for i, size in enumerate(((40, 24), (17, 33))):
        PIL.Image.new('RGB', size, (10 * i, 20, 30)).save(str(d / f'p{i}.png'))
    (d / 'notes.txt').write_text('x')
    spec, enc, files, scale = go.ip_options('a.bin', 'random:clip-tiny', str(d), None)
    assert (spec, enc, scale) == ('a.bin', 'random:clip-tiny', 1.0) and [os.path.basename(f) for f in files] == ['p0.png', 'p1.png']
    assert go.ip_options('a.bin', 'random:clip-tiny', str(d), 0.25)[3] == 0.25
    im = go.load_ip_image(files[1])
    assert im.shape == (3, 33, 17) and im.dtype.name == 'uint8'
    names = {p.name for p in go.main.params}
    assert {'ip_adapter', 'ip_image_encoder', 'ip_images', 'ip_scale'} <= names


def test_sampler_signatures_carry_ip_next_to_control():
    import inspect
    from sid_lsg_amd import sd_util
    from sid_lsg_amd.unet import HipUNet2DCondition
    for fn in (sd_util.sid_sd_sampler, sd_util.hip_generate, sd_util.teacher_sample_i2i, sd_util.teacher_sample_solver_i2i, HipUNet2DCondition.forward_nhwc):
        p = list(inspect.signature(fn).parameters)
        assert p[p.index('control') + 1] == 'ip' and inspect.signature(fn).parameters['ip'].default is None
    for fn in (sd_util.teacher_sample, sd_util.teacher_sample_solver):
        assert 'ip' not in inspect.signature(fn).parameters and 'control' not in inspect.signature(fn).parameters


# ---- precondition of the GPU tolerances ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['tiny40', 'tiny21'])
def test_the_seeded_adapter_changes_the_reference_output_by_more_than_ten_percent(name):
    unet, ad, _, _ = ir.make_ref(name)
    x, t, ctx, emb = ir.make_inputs(name)
    plain, out = ir.ref_outputs(unet, ad, x, t, ctx, emb, 1.0)
    effect = float((out - plain).norm() / plain.norm())
    _, half = ir.ref_outputs(unet, ad, x, t, ctx, emb, 0.5)
    print(f'{name}: image prompt at scale 1 changes the fp64 UNet output by {effect:.3f} (rel. l2), at scale 0.5 by {float((half - plain).norm() / plain.norm()):.3f}')
    assert effect > 0.10
    assert float((half - plain).norm()) > 0 and not torch.allclose(half, out)
    # the unconditional rule: zero embeddings still give non-zero tokens (bias and LayerNorm act)
    assert float(ad.image_proj(torch.zeros(1, ir.EMBED_DIM, dtype=F64)).abs().max()) > 0.1
