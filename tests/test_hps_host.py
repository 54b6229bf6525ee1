"""HPSv2 on the host: Pillow's 8-bit BICUBIC resampling restated in integers against Pillow's own pictures
(tests/golden/hps_ref.npz, tools/make_hps_goldens.py), the geometry rules of the transform, the open_clip checkpoint mapping, the
benchmark prompt lists, the aggregation and the command-line surface."""
import inspect
import json

import numpy as np
import pytest
import torch

from hps_ref_util import CASES, GEOMETRY, STYLES, golden, open_clip_state, pixel_values, write_checkpoint, write_prompts, write_tokenizer


@pytest.fixture(scope='module')
def ref(golden_dir):
    return golden(golden_dir)


# ---- the resampling ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,B,H,W,R,P', CASES, ids=[c[0] for c in CASES])
def test_integer_restatement_reproduces_the_stored_pillow_pictures(ref, name, B, H, W, R, P):
    from sid_lsg_amd import metrics
    src, want = ref[f'src/{name}'], ref[f'pil/{name}']
    assert src.shape == (B, 3, H, W) and want.shape == (B, 3, R, R)
    for b in range(B):
        got = metrics.pil_resize_crop_u8(src[b], R)
        assert got.dtype == np.uint8 and np.array_equal(got, want[b]), (name, b)
    assert (want == 0).any() and (want == 255).any(), 'the case reaches both clamps'


@pytest.mark.parametrize('name,B,H,W,R,P', CASES, ids=[c[0] for c in CASES])
def test_integer_restatement_reproduces_live_pillow(ref, name, B, H, W, R, P):
    Image = pytest.importorskip('PIL.Image')
    from sid_lsg_amd import metrics
    src = ref[f'src/{name}'][0]
    (h, w), (top, left) = GEOMETRY[name]
    im = Image.fromarray(np.ascontiguousarray(src.transpose(1, 2, 0)), 'RGB').resize((w, h), Image.BICUBIC)
    want = np.asarray(im.crop((left, top, left + R, top + R))).transpose(2, 0, 1)
    assert np.array_equal(metrics.pil_resize_crop_u8(src, R), want)


@pytest.mark.parametrize('name,B,H,W,R,P', CASES, ids=[c[0] for c in CASES])
def test_geometry_rules(name, B, H, W, R, P):
    from sid_lsg_amd import metrics
    resized, crop = GEOMETRY[name]
    assert metrics.pil_resized_size(H, W, R) == resized
    assert (metrics.pil_crop_offset(resized[0], R), metrics.pil_crop_offset(resized[1], R)) == crop
    plan = metrics.pil_crop_plan(H, W, R, P)
    assert plan['resized'] == resized and plan['crop'] == crop
    for b, c, side in ((plan['hbounds'], plan['hcoef'], W), (plan['vbounds'], plan['vcoef'], H)):
        assert b.dtype == np.int32 and c.dtype == np.int32 and b.shape == (R, 2) and c.shape[0] == R
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= side).all() and (b[:, 1] <= c.shape[1]).all()
        assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all(), 'the windows move monotonically'
        # weights normalised to 1 and rounded to 22 bits one by one: the sum is 2^22 up to one unit per tap
        assert (np.abs(c.astype(np.int64).sum(1) - (1 << 22)) <= c.shape[1]).all()
        assert int(np.abs(c.astype(np.int64)).sum(1).max()) * 255 + (1 << 21) < 2 ** 31, 'int32 accumulation is exact'
    # band_rows covers every band's source rows
    vb = plan['vbounds']
    for g in range(R // P):
        rows = vb[g * P:(g + 1) * P]
        assert (rows[:, 0] + rows[:, 1]).max() - rows[:, 0].min() <= plan['band_rows']


def test_coefficient_bank_properties():
    from sid_lsg_amd import metrics
    b, c = metrics._bicubic_coefficients(32, 32)
    assert c.shape == (32, 1) and (c == 1 << 22).all() and (b[:, 0] == np.arange(32)).all() and (b[:, 1] == 1).all()
    b, c = metrics._bicubic_coefficients(512, 224)
    assert int(b[:, 1].max()) == 10, 'at most 10 taps per pass at 512 -> 224'
    assert (c < 0).any(), 'the cubic has negative lobes: overshoot exists'
    b, c = metrics._bicubic_coefficients(24, 32)
    assert int(b[:, 1].max()) <= 5 and c.shape[1] == 5                 # up-scaling: support 2, ksize 2 * 2 + 1


def test_production_band_fits_the_lds_limit():
    from sid_lsg_amd import metrics, ops
    for side in (512, 768, 1024):
        plan = metrics.pil_crop_plan(side, side, 224, 14)
        assert 3072 + 3 * plan['band_rows'] * 224 <= ops.PIL_LDS_LIMIT, side


# ---- the checkpoint mapping -----------------------------------------------------------------------------------------------------------
def _expected_transformers(oc):
    """The transformers tensors of the golden model, written out independently of the code under test."""
    want = {'vision_model.embeddings.patch_embedding.weight': oc['visual.conv1.weight'],
            'vision_model.embeddings.class_embedding': oc['visual.class_embedding'],
            'vision_model.embeddings.position_embedding.weight': oc['visual.positional_embedding'],
            'visual_projection.weight': oc['visual.proj'].t(), 'text_projection.weight': oc['text_projection'].t(),
            'text_model.embeddings.token_embedding.weight': oc['token_embedding.weight'],
            'text_model.embeddings.position_embedding.weight': oc['positional_embedding']}
    for p in ('weight', 'bias'):
        want[f'vision_model.pre_layrnorm.{p}'] = oc[f'visual.ln_pre.{p}']
        want[f'vision_model.post_layernorm.{p}'] = oc[f'visual.ln_post.{p}']
        want[f'text_model.final_layer_norm.{p}'] = oc[f'ln_final.{p}']
        for hf, src in (('vision_model', 'visual.transformer'), ('text_model', 'transformer')):
            for i in range(2):
                fused = oc[f'{src}.resblocks.{i}.attn.in_proj_{p}']
                q, k, v = fused[:64], fused[64:128], fused[128:]
                lay = f'{hf}.encoder.layers.{i}.'
                want.update({lay + f'self_attn.q_proj.{p}': q, lay + f'self_attn.k_proj.{p}': k, lay + f'self_attn.v_proj.{p}': v,
                             lay + f'self_attn.out_proj.{p}': oc[f'{src}.resblocks.{i}.attn.out_proj.{p}'],
                             lay + f'layer_norm1.{p}': oc[f'{src}.resblocks.{i}.ln_1.{p}'], lay + f'layer_norm2.{p}': oc[f'{src}.resblocks.{i}.ln_2.{p}'],
                             lay + f'mlp.fc1.{p}': oc[f'{src}.resblocks.{i}.mlp.c_fc.{p}'], lay + f'mlp.fc2.{p}': oc[f'{src}.resblocks.{i}.mlp.c_proj.{p}']})
    return want


def test_open_clip_mapping_is_exact(ref):
    from sid_lsg_amd import clip
    oc = open_clip_state(ref)
    assert 'logit_scale' in oc
    want = _expected_transformers(oc)
    for wrapped in (oc, {'state_dict': {'module.' + k: v for k, v in oc.items()}}, dict(oc, attn_mask=torch.zeros(16, 16))):
        got, cfg = clip.open_clip_to_transformers(wrapped, 'tiny')
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k
    assert set(clip.vision_keys(clip.parse_clip_config(cfg)[0])) <= set(got)
    v, t = clip.parse_clip_config(cfg)
    assert (v.hidden_size, v.intermediate_size, v.num_hidden_layers, v.num_attention_heads, v.image_size, v.patch_size, v.hidden_act) == \
        (64, 128, 2, 2, 32, 8, 'gelu')
    assert (t.hidden_size, t.intermediate_size, t.num_hidden_layers, t.num_attention_heads, t.vocab_size, t.max_position_embeddings,
            t.eos_token_id, t.projection_dim) == (64, 128, 2, 2, 64, 16, 63, 32)


def test_mapped_text_tower_reproduces_the_golden_text_embeddings(ref):
    """The torch text tower under the mapped weights, on the CPU, against transformers' text_embeds: fp32 arithmetic of a 2-layer
    network in another summation order (the bound of tests/test_clip_host.py's text check)."""
    from sid_lsg_amd import clip
    state, cfg = clip.open_clip_to_transformers(open_clip_state(ref), 'tiny')
    _, t = clip.parse_clip_config(cfg)
    text = clip._text_tower(t, 'cpu')
    text.load_state_dict({k: state[k] for k in text.state_dict()})
    det = clip.HipCLIPDetector(type('V', (), {'device': torch.device('cpu'), 'preprocess': 'pil'})(), text.float().eval(), state['text_projection.weight'],
                               None, t.eos_token_id)
    emb = torch.nn.functional.normalize(det.text_embeds_from_ids(torch.from_numpy(ref['ids'])), dim=-1)
    torch.testing.assert_close(emb, torch.from_numpy(ref['text_embeds']), rtol=1e-4, atol=1e-5)


def test_open_clip_mapping_refusals(ref):
    from sid_lsg_amd import clip
    oc = open_clip_state(ref)
    for key in ('visual.conv1.weight', 'visual.proj', 'text_projection', 'ln_final.bias', 'visual.transformer.resblocks.1.mlp.c_fc.weight',
                'transformer.resblocks.0.attn.in_proj_bias', 'token_embedding.weight'):
        with pytest.raises(KeyError, match=key.replace('.', r'\.')):
            clip.open_clip_to_transformers({k: v for k, v in oc.items() if k != key}, 'tiny')
    with pytest.raises(ValueError, match='ViT-H-14.*1280|1280.*ViT-H-14'):
        clip.open_clip_to_transformers(oc, 'ViT-H-14')                       # the table says width 1280, conv1 has 64
    with pytest.raises(ValueError, match='expected one of'):
        clip.open_clip_to_transformers(oc, 'ViT-B-32')
    bad = dict(oc)
    bad['visual.positional_embedding'] = oc['visual.positional_embedding'][:-1]
    with pytest.raises(ValueError, match=r'visual\.positional_embedding'):
        clip.open_clip_to_transformers(bad, 'tiny')
    bad = dict(oc)
    bad['transformer.resblocks.1.attn.in_proj_weight'] = oc['transformer.resblocks.1.attn.in_proj_weight'][:128]
    with pytest.raises(ValueError, match=r'transformer\.resblocks\.1\.attn\.in_proj_weight'):
        clip.open_clip_to_transformers(bad, 'tiny')
    bad = dict(oc)
    bad['token_embedding.weight'] = oc['token_embedding.weight'][:, :32]
    with pytest.raises(ValueError, match=r'token_embedding\.weight'):
        clip.open_clip_to_transformers(bad, 'tiny')
    table = dict(clip.OPEN_CLIP_ARCHS['tiny'], vision_heads=3)
    clip.OPEN_CLIP_ARCHS['tiny3'] = table
    try:
        with pytest.raises(ValueError, match='3 vision heads'):
            clip.open_clip_to_transformers(oc, 'tiny3')
    finally:
        del clip.OPEN_CLIP_ARCHS['tiny3']


def test_load_open_clip_refuses_missing_files(ref, tmp_path):
    from sid_lsg_amd import clip
    tok = write_tokenizer(tmp_path / 'tok')
    with pytest.raises(FileNotFoundError, match='missing.pt'):
        clip.load_open_clip(str(tmp_path / 'missing.pt'), tok, 'cpu', arch='tiny')
    ck = write_checkpoint(ref, tmp_path / 'm.pt')
    with pytest.raises(FileNotFoundError, match='vocab.json'):
        clip.load_open_clip(ck, str(tmp_path / 'nowhere'), 'cpu', arch='tiny')
    with pytest.raises(ValueError, match='text_tower'):
        clip.load_open_clip(ck, tok, 'cpu', arch='tiny', text_tower='jax')
    det = clip.load_open_clip(ck, tok, 'cpu', arch='tiny')                 # construction needs no GPU; running the tower does
    assert det.preprocess == 'pil' and det.tokenizer.eos_token_id == 63 and det.tokenizer.model_max_length == 16
    with torch.no_grad(), pytest.raises(RuntimeError, match='MI355X'):
        det.vision(torch.zeros(1, 3, 40, 40, dtype=torch.uint8))
    assert clip.load_open_clip(write_checkpoint(ref, tmp_path / 'w.bin', wrap=True), tok, 'cpu', arch='tiny').vision.cfg.image_size == 32
    assert clip.load_open_clip(write_checkpoint(ref, tmp_path / 'm.safetensors'), tok, 'cpu', arch='tiny', preprocess='interpolate').preprocess == 'interpolate'
    with pytest.raises(ValueError, match='preprocess'):
        clip.load_open_clip(ck, tok, 'cpu', arch='tiny', preprocess='lanczos')


def test_preprocess_selection_and_arch_table():
    from sid_lsg_amd import clip
    assert inspect.signature(clip.HipCLIPVisionTower.__init__).parameters['preprocess'].default == 'interpolate'
    assert inspect.signature(clip.load_clip).parameters['preprocess'].default == 'interpolate'
    v, t = clip.parse_clip_config(clip.CLIP_ARCHS['vit-h-14'])
    assert (v.hidden_size, v.num_attention_heads, v.num_hidden_layers, v.hidden_act) == (1280, 16, 32, 'gelu')
    assert v.hidden_size // v.num_attention_heads == 80 and (t.hidden_size, t.num_hidden_layers) == (1024, 24)
    assert set(clip.OPEN_CLIP_ARCHS) >= {'ViT-H-14', 'ViT-L-14', 'ViT-g-14', 'tiny'}


# ---- prompts, aggregation -------------------------------------------------------------------------------------------------------------
def test_benchmark_prompts(tmp_path):
    from sid_lsg_amd import hps
    assert hps.STYLES == STYLES
    d, want = write_prompts(tmp_path / 'p', 5)
    assert hps.benchmark_prompts(d) == want
    (tmp_path / 'p' / 'paintings.json').unlink()
    with pytest.raises(FileNotFoundError, match='paintings.json'):
        hps.benchmark_prompts(d)
    (tmp_path / 'p' / 'paintings.json').write_text(json.dumps({'a': 1}))
    with pytest.raises(ValueError, match='paintings.json'):
        hps.benchmark_prompts(d)
    with pytest.raises(FileNotFoundError, match='not a directory'):
        hps.benchmark_prompts(str(tmp_path / 'none'))


def test_aggregate_on_hand_made_scores():
    from sid_lsg_amd import hps
    scores = {}
    for j, style in enumerate(STYLES):
        scores[style] = [0.20 + 0.01 * j] * 80 + [0.30 + 0.01 * j] * 80          # two groups of 80: means 0.20 + .., 0.30 + ..
    res = hps.aggregate(scores)
    for j, style in enumerate(STYLES):
        assert res[style] == pytest.approx(25.0 + j, abs=1e-9)
        assert res[style + '_std'] == pytest.approx(5.0, abs=1e-9)               # population std of (a, a + 0.1) is 0.05
    assert res['Average'] == pytest.approx(26.5, abs=1e-9)
    one = hps.aggregate({'photo': [0.25] * 80 + [0.35] * 40})                    # a short last group is a group of its own
    assert one['photo'] == pytest.approx(100 * (0.25 * 80 + 0.35 * 40) / 120) and one['photo_std'] == pytest.approx(5.0)
    with pytest.raises(ValueError, match='anime'):
        hps.aggregate({'anime': []})
    assert 'Average' in hps.format_table(res) and 'concept-art' in hps.format_table(res)


def test_jpeg_round_trip_is_pils():
    Image = pytest.importorskip('PIL.Image')
    import io
    from sid_lsg_amd import hps
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (2, 3, 24, 32), generator=g, dtype=torch.uint8)
    back = hps.jpeg_round_trip(img)
    assert back.shape == img.shape and back.dtype == torch.uint8
    buf = io.BytesIO()
    Image.fromarray(img[1].permute(1, 2, 0).numpy(), 'RGB').save(buf, format='JPEG')
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB')), back[1].permute(1, 2, 0).numpy())
    assert hps.image_path('o', 'photo', 1234, subdirs=True).replace('\\', '/') == 'o/photo/001000/01234.jpg'
    assert hps.image_path('o', 'anime', 7).replace('\\', '/') == 'o/anime/00007.jpg'


# ---- metric registry and command lines -------------------------------------------------------------------------------------------------
def test_hpsv2_is_a_registered_metric():
    from sid_lsg_amd import metrics
    assert metrics.is_valid_metric('hpsv2') and metrics.is_valid_metric('hpsv2_test')
    assert metrics.list_valid_metrics()[:4] == ['fid30k_full', 'fid_clip_30k_full', 'fid_test', 'fid_clip_test']
    assert metrics.HPS_METRICS == ('hpsv2', 'hpsv2_test')
    opts = metrics.MetricOptions(G=None, device='cpu', metric_hps_path='m.pt', hps_prompts='p', hps_arch='tiny', hps_tokenizer='t')
    assert (opts.metric_hps_path, opts.hps_prompts, opts.hps_arch, opts.hps_tokenizer) == ('m.pt', 'p', 'tiny', 't')
    with pytest.raises(ValueError, match='--metric_hps_path'):
        metrics.calc_metric('hpsv2_test', G=None, prompts=['a'], device='cpu')


def test_hps_options_reach_the_loop(tmp_path):
    import click
    import sid_train
    from sid_lsg_amd.training_loop import _hps_opt, evaluate_network, evaluate_teacher, training_loop
    for fn in (training_loop, evaluate_network, evaluate_teacher):
        for k in ('metric_hps_path', 'hps_prompts', 'hps_arch', 'hps_tokenizer'):
            assert inspect.signature(fn).parameters[k].default is None
    assert _hps_opt(None, None, None, None, 'random:tiny') == {}
    assert _hps_opt('m.pt', 'p', None, None, '/models/sd15')['hps_tokenizer'].replace('\\', '/') == '/models/sd15/tokenizer'
    flags = {f[0] for f, _ in sid_train.OPTIONS}
    assert {'--metric_hps_path', '--hps_prompts', '--hps_arch', '--hps_tokenizer'} <= flags
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a red cube\n')
    ck = tmp_path / 'm.pt'
    ck.write_bytes(b'x')
    prompts, _ = write_prompts(tmp_path / 'p', 2)
    o = dict(outdir='x', data=None, data_stat=None, data_prompt_text=str(tmp_path), duration=0.01, batch=8, batch_gpu=2, ema=0.05, xflip=0.0,
             bench=True, cache=True, workers=1, desc=None, nosubdir=False, tick=2, snap=50, dump=100, seed=3, transfer=None, resume=None,
             dry_run=True, metrics=['hpsv2_test'], sd_model='random:tiny', resolution=64, init_timestep=625, fp16=False, ls=1, lsg=1, alpha=1,
             tmax=980, tmin=20, lr=1e-6, glr=2e-6, train_mode=False, network_pkl='teacher', cfg_train_fake=1.5, cfg_eval_fake=1.5,
             cfg_eval_real=1.5, metric_pt_path=None, metric_clip_path=None, metric_open_clip_path=None, enable_xformers=True,
             gradient_checkpointing=False, optimizer='adam', num_steps=1, fake_score_use_lora=False, metric_hps_path=str(ck),
             hps_prompts=prompts, hps_arch='tiny', hps_tokenizer=None)
    c = sid_train.build_config(sid_train.EasyDict(o))                      # no Inception file, no statistics: hpsv2 needs neither
    assert c.metric_hps_path == str(ck) and c.hps_prompts == prompts and c.hps_arch == 'tiny' and 'hps_tokenizer' not in c
    inspect.signature(training_loop).bind(**c)
    with pytest.raises(click.ClickException, match='--metric_hps_path'):
        sid_train.build_config(sid_train.EasyDict(dict(o, metric_hps_path=None)))
    with pytest.raises(click.ClickException, match='--hps_prompts'):
        sid_train.build_config(sid_train.EasyDict(dict(o, hps_prompts=str(tmp_path / 'none'))))
    with pytest.raises(click.ClickException, match='--metric_pt_path'):
        sid_train.build_config(sid_train.EasyDict(dict(o, metrics=['hpsv2_test', 'fid_test'])))


def test_generate_hpsv2_option_parsing(ref, tmp_path):
    from click.testing import CliRunner
    import generate_hpsv2
    params = {p.name: p for p in generate_hpsv2.main.params}
    assert params['seeds'].default == '0-799' and params['max_batch_size'].default == 16 and params['init_timestep'].default == 625
    assert params['hps_arch'].default == 'ViT-H-14' and params['score_only'].is_flag and params['subdirs'].is_flag
    for name in ('network_pkl', 'outdir', 'num_fid_samples', 'repo_id', 'resolution', 'num_steps_eval', 'text_encoder', 'hps_prompts',
                 'hps_checkpoint', 'hps_tokenizer'):
        assert name in params, name
    prompts, _ = write_prompts(tmp_path / 'p', 4)
    tok = write_tokenizer(tmp_path / 'tok')
    ck = write_checkpoint(ref, tmp_path / 'm.pt')
    base = ['--outdir', str(tmp_path / 'out'), '--repo_id', 'random:tiny', '--hps_arch', 'tiny']
    run = lambda extra: CliRunner().invoke(generate_hpsv2.main, base + extra)      # noqa: E731
    # every refusal below happens before the GPU is touched
    r = run(['--network', 'teacher', '--hps_checkpoint', ck, '--hps_tokenizer', tok])
    assert r.exit_code != 0 and '--hps_prompts' in r.output
    r = run(['--network', 'teacher', '--hps_prompts', prompts, '--hps_tokenizer', tok])
    assert r.exit_code != 0 and '--hps_checkpoint' in r.output
    r = run(['--network', 'teacher', '--hps_prompts', prompts, '--hps_checkpoint', ck])
    assert r.exit_code != 0 and 'vocab.json' in r.output and 'random:tiny' in r.output          # the default: <repo_id>/tokenizer
    r = run(['--hps_prompts', prompts, '--hps_checkpoint', ck, '--hps_tokenizer', tok])
    assert r.exit_code != 0 and '--network' in r.output
    r = run(['--network', 'teacher', '--hps_prompts', prompts, '--hps_checkpoint', ck, '--hps_tokenizer', tok])
    assert r.exit_code != 0 and 'seed 4 has no prompt' in r.output                               # 0-799 against 4 prompts per style
    r = run(['--network', 'teacher', '--hps_prompts', prompts, '--hps_checkpoint', ck, '--hps_tokenizer', tok, '--resolution', '60'])
    assert r.exit_code != 0 and 'multiple of 8' in r.output
    r = run(['--network', str(tmp_path / 'snap.pkl'), '--teacher_steps', '3', '--hps_prompts', prompts, '--hps_checkpoint', ck, '--hps_tokenizer', tok])
    assert r.exit_code != 0 and 'teacher' in r.output
    (tmp_path / 'p' / 'photo.json').unlink()
    r = run(['--network', 'teacher', '--hps_prompts', prompts, '--hps_checkpoint', ck, '--hps_tokenizer', tok])
    assert r.exit_code != 0 and 'photo.json' in r.output
