"""LoRA loading, host side (no GPU): the two key families, alpha / rank, the physical layout of the factors, concatenation and padding
along the rank, every refusal, the option checks of both command lines, the amplitude of random:lora and the job table."""
import json

import numpy as np
import pytest
import torch

import lora_ref

TINY_TE = dict(hidden=64, layers=2, heads=2, dff=128, max_pos=13, act='quick_gelu')


@pytest.fixture(scope='module')
def nets():
    """random:tiny without a device: the unmaterialised UNet (names and shapes), its seeded weights as a state dict, the text encoder."""
    from sid_lsg_amd.text import CLIPTextModel
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition, random_state_dict
    g = torch.random.get_rng_state()
    torch.manual_seed(1)
    te = CLIPTextModel(**TINY_TE).requires_grad_(False)
    torch.random.set_rng_state(g)
    cfg = CONFIGS['tiny']
    return HipUNet2DCondition(cfg), random_state_dict(cfg, 0), te


@pytest.fixture(scope='module')
def rnd(nets):
    from sid_lsg_amd import lora
    unet, usd, te = nets
    return lora.random_lora_state_dict(unet, te, rank=4, seed=0, unet_state=usd)


def _same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) and x[3] == y[3] and x[4] == y[4]
                                    for x, y in zip(a, b))


def test_random_lora_covers_every_target_with_kohya_keys(nets, rnd):
    from sid_lsg_amd import lora
    unet, usd, te = nets
    table = lora.layer_table(unet, te)
    kinds = {L.kind for L in table.values()}
    assert kinds == {'linear', 'conv1x1', 'conv3x3'}
    for want in ('conv_in', 'conv_out', 'time_embedding.linear_1', 'down_blocks.0.resnets.0.time_emb_proj', 'down_blocks.0.resnets.0.conv1',
                 'down_blocks.1.resnets.0.conv_shortcut', 'down_blocks.0.downsamplers.0.conv', 'up_blocks.0.upsamplers.0.conv',
                 'down_blocks.0.attentions.0.proj_in', 'down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k',
                 'down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_out.0', 'down_blocks.0.attentions.0.transformer_blocks.0.ff.net.0.proj',
                 'down_blocks.0.attentions.0.transformer_blocks.0.ff.net.2'):
        assert ('unet', want) in table, want
    assert ('te', 'text_model.encoder.layers.1.mlp.fc2') in table and ('te', 'text_model.encoder.layers.0.self_attn.q_proj') in table
    assert all(k.startswith(('lora_unet_', 'lora_te_')) for k in rnd)
    parsed = lora.parse_lora(rnd, unet, te)
    assert [p[0] for p in parsed] == list(table)
    assert all(float(p[1].abs().min()) > 0 or p[1].numel() > 1 for p in parsed) and all(float(p[1].norm()) > 0 and float(p[2].norm()) > 0 for p in parsed)


def test_both_key_families_give_the_same_adapters(nets, rnd):
    from sid_lsg_amd import lora
    unet, usd, te = nets
    a = lora.parse_lora(rnd, unet, te)
    for style in ('peft', 'old'):
        b = lora.parse_lora(lora_ref.kohya_to_diffusers(rnd, usd, te.state_dict(), style), unet, te)
        assert _same(a, b), style


def test_alpha_over_rank_and_the_missing_alpha(nets):
    from sid_lsg_amd import lora
    unet, usd, te = nets
    name = 'mid_block.attentions.0.transformer_blocks.0.attn1.to_q'
    head = 'lora_unet_' + name.replace('.', '_')
    g = torch.Generator().manual_seed(5)
    down, up = torch.randn(8, 128, generator=g), torch.randn(128, 8, generator=g)
    with_alpha = lora.parse_lora({head + '.lora_down.weight': down, head + '.lora_up.weight': up, head + '.alpha': torch.tensor(2.0)}, unet, te)
    without = lora.parse_lora({head + '.lora_down.weight': down, head + '.lora_up.weight': up}, unet, te)
    assert with_alpha[0][3] == 2.0 and with_alpha[0][4] == 8 and without[0][3] == 8.0
    table = lora.layer_table(unet, te)
    assert lora.HostPlan('unet', table, [with_alpha]).layers[0]['cols'] == [(0, 0, 8, 0.25)]
    assert lora.HostPlan('unet', table, [without]).layers[0]['cols'] == [(0, 0, 8, 1.0)]
    coef = lora.HostPlan('unet', table, [with_alpha]).coef([3.0])
    assert coef.dtype == torch.float32 and torch.equal(coef, torch.full((8,), 0.75))
    # the diffusers family: no alpha -> scale 1, i.e. alpha = rank
    dif = lora.parse_lora({f'unet.{name}.lora_A.weight': down, f'unet.{name}.lora_B.weight': up}, unet, te)
    assert dif[0][3] == 8.0


def test_conv3x3_down_is_permuted_to_r_3_3_cin(nets):
    from sid_lsg_amd import lora
    unet, usd, te = nets
    g = torch.Generator().manual_seed(2)
    cin, cout, r = 4, 32, 3          # conv_in of tiny
    down, up = torch.randn(r, cin, 3, 3, generator=g), torch.randn(cout, r, 1, 1, generator=g)
    ad = lora.parse_lora({'lora_unet_conv_in.lora_down.weight': down, 'lora_unet_conv_in.lora_up.weight': up}, unet, te)
    plan = lora.HostPlan('unet', lora.layer_table(unet, te), [ad])
    L = plan.layers[0]
    assert (L['layer'].n, L['layer'].kk, L['r'], L['rp']) == (cout, 36, 3, 4)
    D = plan.down[L['down_off']:L['down_off'] + 4 * 36].view(4, 3, 3, cin)
    for rr in range(r):
        for kh in range(3):
            for kw in range(3):
                for c in range(cin):
                    assert D[rr, kh, kw, c] == down[rr, c, kh, kw]
    assert float(D[3].abs().max()) == 0
    U = plan.up[L['up_off']:L['up_off'] + cout * 4].view(cout, 4)
    assert torch.equal(U[:, :3], up.view(cout, r)) and float(U[:, 3].abs().max()) == 0
    # and the merged master in its physical layout equals the reference's diffusers-layout result, permuted
    merged, _ = lora_ref.merge(usd, {}, [{'lora_unet_conv_in.lora_down.weight': down, 'lora_unet_conv_in.lora_up.weight': up}], [1.0])
    mine = usd['conv_in.weight'].double().permute(0, 2, 3, 1).reshape(cout, 36) + (U.double() * plan.coef([1.0]).double()) @ plan.down[:4 * 36].view(4, 36).double()
    assert torch.allclose(mine, merged['conv_in.weight'].permute(0, 2, 3, 1).reshape(cout, 36), rtol=0, atol=1e-12)


def test_two_files_on_one_layer_concatenate_along_the_rank_and_pad_to_4(nets):
    from sid_lsg_amd import lora
    unet, usd, te = nets
    name = 'down_blocks.0.attentions.0.proj_in'         # a 1 x 1 convolution: factors may be 2-D or 4-D
    head = 'lora_unet_' + name.replace('.', '_')
    g = torch.Generator().manual_seed(3)
    f1 = {head + '.lora_down.weight': torch.randn(3, 32, 1, 1, generator=g), head + '.lora_up.weight': torch.randn(32, 3, 1, 1, generator=g),
          head + '.alpha': torch.tensor(6.0)}
    f2 = {head + '.lora_down.weight': torch.randn(2, 32, generator=g), head + '.lora_up.weight': torch.randn(32, 2, generator=g)}
    ads = [lora.parse_lora(f, unet, te) for f in (f1, f2)]
    plan = lora.HostPlan('unet', lora.layer_table(unet, te), ads)
    L = plan.layers[0]
    assert (L['r'], L['rp']) == (5, 8) and L['cols'] == [(0, 0, 3, 2.0), (1, 3, 5, 1.0)]
    coef = plan.coef([0.5, -3.0])
    assert coef.tolist() == [1.0, 1.0, 1.0, -3.0, -3.0, 0.0, 0.0, 0.0]
    U, D = plan.up.view(32, 8), plan.down.view(8, 32)
    assert torch.equal(U[:, :3], f1[head + '.lora_up.weight'].view(32, 3)) and torch.equal(U[:, 3:5], f2[head + '.lora_up.weight'])
    assert torch.equal(D[3:5], f2[head + '.lora_down.weight']) and float(D[5:].abs().max()) == 0 and float(U[:, 5:].abs().max()) == 0
    merged, _ = lora_ref.merge(usd, {}, [f1, f2], [0.5, -3.0])
    mine = usd[name + '.weight'].double().view(32, 32) + (U.double() * coef.double()) @ D.double()
    assert torch.allclose(mine, merged[name + '.weight'].view(32, 32), rtol=0, atol=1e-12)


def _pair(head, r=4, cin=128, cout=128):
    return {head + '.lora_down.weight': torch.ones(r, cin), head + '.lora_up.weight': torch.ones(cout, r)}


Q = 'lora_unet_mid_block_attentions_0_transformer_blocks_0_attn1_to_q'


@pytest.mark.parametrize('sd, key', [
    ({Q + '.hada_w1_a': torch.ones(4, 4)}, Q + '.hada_w1_a'),
    ({Q + '.lokr_w1': torch.ones(4, 4)}, Q + '.lokr_w1'),
    ({**_pair(Q), Q + '.dora_scale': torch.ones(1, 128)}, Q + '.dora_scale'),
    ({**_pair(Q), Q + '.lora_mid.weight': torch.ones(4, 4, 3, 3)}, Q + '.lora_mid.weight'),
    ({Q + '.diff': torch.ones(128, 128)}, Q + '.diff'),
    ({Q + '.diff_b': torch.ones(128)}, Q + '.diff_b'),
    (_pair('lora_te1_text_model_encoder_layers_0_mlp_fc1'), 'lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_down.weight'),
    (_pair('lora_te2_text_model_encoder_layers_0_mlp_fc1'), 'lora_te2_text_model_encoder_layers_0_mlp_fc1.lora_down.weight'),
    (_pair('lora_unet_input_blocks_1_1_proj_in'), 'lora_unet_input_blocks_1_1_proj_in.lora_down.weight'),
    (_pair('lora_unet_middle_block_1_proj_in'), 'lora_unet_middle_block_1_proj_in.lora_down.weight'),
    (_pair('lora_unet_output_blocks_3_1_proj_in'), 'lora_unet_output_blocks_3_1_proj_in.lora_down.weight'),
    (_pair('lora_unet_mid_block_attentions_0_transformer_blocks_0_attn3_to_q'), 'lora_unet_mid_block_attentions_0_transformer_blocks_0_attn3_to_q.lora_down.weight'),
    ({'unet.mid_block.attentions.0.nowhere.lora_A.weight': torch.ones(4, 128)}, 'unet.mid_block.attentions.0.nowhere.lora_A.weight'),
    ({Q + '.lora_up.weight': torch.ones(128, 4)}, Q + '.lora_up.weight'),
    ({Q + '.lora_down.weight': torch.ones(4, 128)}, Q + '.lora_down.weight'),
    ({Q + '.lora_down.weight': torch.ones(4, 64), Q + '.lora_up.weight': torch.ones(128, 4)}, Q + '.lora_down.weight'),
    ({Q + '.lora_down.weight': torch.ones(4, 128), Q + '.lora_up.weight': torch.ones(128, 8)}, Q + '.lora_up.weight'),
    ({Q + '.lora_down.weight': torch.ones(4, 128, 3, 3), Q + '.lora_up.weight': torch.ones(128, 4)}, Q + '.lora_down.weight'),
    ({'lora_unet_conv_in.lora_down.weight': torch.ones(4, 4), 'lora_unet_conv_in.lora_up.weight': torch.ones(32, 4, 1, 1)}, 'lora_unet_conv_in.lora_down.weight'),
    ({Q + '.lora_down.weight': torch.ones(0, 128), Q + '.lora_up.weight': torch.ones(128, 0)}, Q + '.lora_down.weight'),
    ({'state_dict.step': torch.ones(1)}, 'state_dict.step'),
])
def test_refusals_name_the_key(nets, sd, key):
    from sid_lsg_amd import lora
    unet, usd, te = nets
    with pytest.raises(ValueError) as e:
        lora.parse_lora(sd, unet, te)
    assert key in str(e.value), str(e.value)


def test_refuses_an_empty_file_and_a_rank_above_4096(nets):
    from sid_lsg_amd import lora
    unet, usd, te = nets
    with pytest.raises(ValueError, match='no LoRA key'):
        lora.parse_lora({}, unet, te, where='empty.safetensors')
    big = lora.parse_lora(_pair(Q, r=2052), unet, te)
    table = lora.layer_table(unet, te)
    lora.HostPlan('unet', table, [big])                    # 2052 alone is fine
    with pytest.raises(ValueError) as e:
        lora.HostPlan('unet', table, [big, big])           # 4104 concatenated is not
    assert 'mid_block.attentions.0.transformer_blocks.0.attn1.to_q' in str(e.value) and '4104' in str(e.value)
    with pytest.raises(ValueError, match='one per file'):
        lora.check_scales([1.0], 2)
    with pytest.raises(ValueError, match='finite'):
        lora.check_scales([float('nan')], 1)


def test_random_spec_and_file_reading(tmp_path, nets, rnd):
    from safetensors.torch import save_file

    from sid_lsg_amd import lora
    assert lora.parse_random_spec('random:lora') == (4, None)
    assert lora.parse_random_spec('random:lora:32') == (32, None) and lora.parse_random_spec('random:lora:8:5') == (8, 5)
    for bad in ('random:lora:x', 'random:lora:0', 'random:lora:4:5:6', 'random:ip-adapter'):
        with pytest.raises(ValueError):
            lora.parse_random_spec(bad)
    small = {k: v for k, v in rnd.items() if k.startswith('lora_te_')}
    save_file(small, str(tmp_path / 'a.safetensors'))
    torch.save(small, str(tmp_path / 'a.pt'))
    for f in ('a.safetensors', 'a.pt'):
        got = lora.read_lora_file(str(tmp_path / f))
        assert set(got) == set(small) and all(torch.equal(got[k], small[k]) for k in small)
    with pytest.raises(FileNotFoundError):
        lora.read_lora_file(str(tmp_path / 'missing.safetensors'))
    (tmp_path / 'a.txt').write_text('x')
    with pytest.raises(ValueError, match='expected a .safetensors'):
        lora.read_lora_file(str(tmp_path / 'a.txt'))


def test_random_lora_amplitude_on_tiny(nets, rnd):
    """|dW|_F / |W|_F within [0.1, 1] for every layer of random:tiny at scale 1, measured on the fp64 reference merge."""
    unet, usd, te = nets
    tsd = te.state_dict()
    mu, mt = lora_ref.merge(usd, tsd, [rnd], [1.0])
    walked = lora_ref.walk(rnd, usd, tsd)
    assert len(walked) > 200
    for net, mod in walked:
        w0 = (usd if net == 'unet' else tsd)[mod + '.weight'].double()
        w1 = (mu if net == 'unet' else mt)[mod + '.weight']
        ratio = float((w1 - w0).norm() / w0.norm())
        assert 0.1 <= ratio <= 1.0, (net, mod, ratio)


def test_job_table_is_sorted_and_gap_free(nets, rnd):
    from sid_lsg_amd import lora, ops
    unet, usd, te = nets
    plan = lora.HostPlan('unet', lora.layer_table(unet, te), [lora.parse_lora(rnd, unet, te)])
    ptrs = [4096 * (i + 1) for i in range(len(plan.layers))]
    table = plan.job_table(ptrs, ptrs, 1 << 30, 1 << 31, 1 << 32, 'cpu')
    rec = table.host
    assert rec.dtype.itemsize == 56 and table.njobs == len(plan.layers) == len(plan.names)
    blk = 0
    for r, L in zip(rec, plan.layers):
        assert int(r['blk0']) == blk and int(r['N']) == L['layer'].n and int(r['KK']) == L['layer'].kk and int(r['R']) == L['rp']
        assert int(r['R']) % 4 == 0 and int(r['KK']) % 4 == 0
        assert int(r['up']) == (1 << 30) + 4 * L['up_off'] and int(r['down']) == (1 << 31) + 4 * L['down_off'] and int(r['coef']) == (1 << 32) + 4 * L['coef_off']
        assert all(int(r[f]) % 16 == 0 for f in ('base', 'dst', 'up', 'down', 'coef'))
        blk += -(-L['layer'].n // 64) * -(-L['layer'].kk // 64)
    assert table.nblocks == blk
    assert np.array_equal(np.frombuffer(table.device.numpy().tobytes(), dtype=rec.dtype), rec)
    assert ops.lora_job_fault(rec, blk, plan.names) is None
    assert 'nblocks' in ops.lora_job_fault(rec, blk + 1, plan.names)
    bad = rec.copy()
    bad['R'][3] = 6
    assert plan.names[3] in ops.lora_job_fault(bad, blk, plan.names)


def test_header_declares_the_entry_point():
    from sid_lsg_amd._lib import parse_header
    protos = parse_header()
    assert 'sidlsg_lora_merge_f32' in protos and len(protos['sidlsg_lora_merge_f32']) == 5
    from sid_lsg_amd.csrc.build import SOURCES
    assert 'lora.hip' in SOURCES


# ------------------------------------------------------------------------------------------------
# command lines
def test_lora_scale_rule():
    from sid_lsg_amd.sd_util import lora_scales
    assert lora_scales(0, ()) == [] and lora_scales(2, ()) == [1.0, 1.0] and lora_scales(3, (0.5,)) == [0.5] * 3
    assert lora_scales(2, (0.5, -1)) == [0.5, -1.0]
    for n, s in ((0, (1.0,)), (3, (1.0, 2.0)), (1, (1.0, 2.0))):
        with pytest.raises(ValueError):
            lora_scales(n, s)


def test_generate_onestep_usage_errors(tmp_path):
    from click.testing import CliRunner

    import generate_onestep as g
    base = ['--network', 'teacher', '--outdir', str(tmp_path / 'o'), '--repo_id', 'random:tiny', '--resolution', '64']
    res = CliRunner().invoke(g.main, base + ['--lora_scale', '0.5'])
    assert res.exit_code == 2 and '--lora_scale applies to --lora only' in res.output, res.output
    res = CliRunner().invoke(g.main, base + ['--lora', 'random:lora', '--lora', 'random:lora:8', '--lora', 'random:lora:4:1', '--lora_scale', '1', '--lora_scale', '2'])
    assert res.exit_code == 2 and '2 --lora_scale values for 3 --lora files' in res.output, res.output
    assert g.lora_options((), ()) is None
    assert g.lora_options(('a', 'b'), (0.5,)) == (['a', 'b'], [0.5, 0.5])
    assert g.lora_options(('a',), (-2.0,)) == (['a'], [-2.0])


def _dry_run(tmp_path, *extra):
    from click.testing import CliRunner

    import sid_train
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a red cube\na blue sphere\n')
    return CliRunner().invoke(sid_train.main, [
        '--outdir', str(tmp_path / 'runs'), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny', '--seed', '3', '--batch', '8',
        '--batch-gpu', '2', '--duration', '0.01', '--dry-run', *extra])


def test_sid_train_dry_run_stores_the_lora_options(tmp_path):
    res = _dry_run(tmp_path, '--lora', 'random:lora', '--lora', 'random:lora:8:2', '--lora_scale', '0.5')
    assert res.exit_code == 0, res.output
    opts = json.loads(res.output[res.output.index('{'):res.output.rindex('}') + 1])
    assert opts['lora'] == {'specs': ['random:lora', 'random:lora:8:2'], 'scales': [0.5, 0.5]}
    plain = _dry_run(tmp_path)
    assert plain.exit_code == 0 and '"lora"' not in plain.output, 'the printed options of a run without the option stay as they were'
    for extra, msg in ((('--lora_scale', '2'), '--lora_scale applies to --lora only'),
                       (('--lora', 'random:lora', '--lora_scale', '1', '--lora_scale', '2'), '2 --lora_scale values for 1 --lora files'),
                       (('--lora', str(tmp_path / 'none.safetensors')), 'not a local file'),
                       (('--fake_score_use_lora', '1'), '--fake_score_use_lora is not supported')):
        bad = _dry_run(tmp_path, *extra)
        assert bad.exit_code != 0 and msg in bad.output, bad.output


def test_training_loop_without_lora_loads_nothing(monkeypatch):
    """_fuse_lora with None or an empty list returns before it touches the networks (plain objects here: any attribute access would
    raise) and before it imports sid_lsg_amd.lora."""
    import sys

    from sid_lsg_amd import training_loop as tl
    monkeypatch.delitem(sys.modules, 'sid_lsg_amd.lora', raising=False)
    sentinel = object()
    for empty in (None, {}, dict(specs=[], scales=[])):
        assert tl._fuse_lora(empty, sentinel, sentinel) is None
    assert 'sid_lsg_amd.lora' not in sys.modules


def test_cost_tool_rewrites_only_its_own_section(tmp_path):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('lora_cost', os.path.join(root, 'tools', 'lora_cost.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / 'lora.txt'
    out.write_text('figures of the tests\nsecond line\n\n' + tool.MARKER + ' (an older run) ==\nold 1\nold 2\n')
    tool.write_section(str(out), ['new 1'])
    text = out.read_text().splitlines()
    assert text[:3] == ['figures of the tests', 'second line', ''] and text[3].startswith(tool.MARKER) and text[4:] == ['new 1']
    fresh = tmp_path / 'sub' / 'fresh.txt'
    tool.write_section(str(fresh), ['only'])
    assert fresh.read_text().splitlines()[1:] == ['only']
