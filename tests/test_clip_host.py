"""CLIP score, host side (no GPU): configuration parsing, key mapping and refusals of sid_lsg_amd.clip.load_clip against a directory
written from tests/golden/clip_ref.npz (tools/make_clip_goldens.py: transformers.CLIPModel on the CPU), the PyTorch text path against
the golden text embeddings, the fp64 restatement of the preprocessing against F.interpolate, and the metric / command-line seams."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clip_ref_util import MEAN, RESIZE_CASES, STD, case_images, golden, pixel_values64, state_dict_of, write_clip_dir

from sid_lsg_amd import clip, metrics


@pytest.fixture(scope='module')
def ref(golden_dir):
    return golden(golden_dir)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_config_and_key_mapping(ref, tag, tmp_path):
    det = clip.load_clip(write_clip_dir(ref, tag, tmp_path / tag), 'cpu')
    cfg = json.loads(str(ref[f'{tag}/config']))
    v = det.vision.cfg
    for f in clip.VISION_FIELDS:
        assert getattr(v, f) == cfg['vision_config'][f], f
    assert v.projection_dim == cfg['projection_dim']
    assert det.vision.tokens == 1 + (v.image_size // v.patch_size) ** 2
    assert det.vision.compute_dtype == torch.bfloat16
    assert clip.load_clip(str(tmp_path / tag), 'cpu', compute_dtype=torch.float32).vision.compute_dtype == torch.float32
    sd = state_dict_of(ref, tag)
    vis = {k for k in sd if k.startswith('vision_model.')} | {'visual_projection.weight'}
    assert set(det.vision.masters) == vis == set(clip.vision_keys(v))
    for k in vis:
        assert det.vision.masters[k].dtype == torch.float32 and torch.equal(det.vision.masters[k], sd[k]), k
    text = det.text_encoder.state_dict()
    assert set(text) == {k for k in sd if k.startswith('text_model.')}
    for k, w in text.items():
        assert torch.equal(w, sd[k]), k
    assert torch.equal(det.text_projection, sd['text_projection.weight'])
    assert det.eos_token_id == 63 and det.tokenizer.eos_token_id == 63 and det.tokenizer.bos_token_id == 62
    assert det.tokenizer.model_max_length == 16
    ids = det.tokenizer(['ab c', 'x' * 40]).input_ids
    assert ids.shape == (2, 16) and int(ids.max()) < 64
    assert ids[0].tolist()[:6] == [62, 1, 28, 29, 63, 63]                  # a, b</w>, c</w>
    assert ids[1, 0] == 62 and ids[1, 15] == 63 and 63 not in ids[1, 1:15].tolist(), 'truncation keeps BOS and EOS'


def test_early_config_eos_and_random_specs():
    cfg = json.loads(json.dumps(clip.CLIP_ARCHS['vit-l-14']))
    cfg['text_config']['eos_token_id'] = 2           # early transformers configs: pooled at argmax(ids) = the first <|endoftext|>
    assert clip.parse_clip_config(cfg)[1].eos_token_id == 49407
    for arch, head in (('tiny', 32), ('vit-l-14', 64), ('vit-g-14', 88)):
        v, _ = clip.parse_clip_config(clip.CLIP_ARCHS[arch])
        assert v.hidden_size // v.num_attention_heads == head
    with pytest.raises(ValueError, match='random:clip-'):
        clip.load_clip('random:clip-nope', 'cpu')
    det = clip.load_clip('random:clip-tiny', 'cpu')
    assert isinstance(det, clip.HipCLIPDetector) and det.tokenizer.model_max_length == 77
    again = clip.load_clip('random:clip-tiny', 'cpu')
    assert all(torch.equal(det.vision.masters[k], again.vision.masters[k]) for k in det.vision.masters), 'seeded'


def _edit(part, field, value):
    def fn(cfg):
        if value is None:
            del cfg[part][field]
        else:
            cfg[part][field] = value
    return fn


@pytest.mark.parametrize('edit,exc,names', [
    (_edit('vision_config', 'hidden_act', 'relu'), ValueError, r'vision_config\.hidden_act'),
    (_edit('text_config', 'hidden_act', 'gelu_new'), ValueError, r'text_config\.hidden_act'),
    (_edit('vision_config', 'num_attention_heads', 16), ValueError, r'vision_config\.num_attention_heads.*head dim 4'),
    (_edit('vision_config', 'image_size', 30), ValueError, r'vision_config\.image_size % patch_size'),
    (_edit('vision_config', 'patch_size', None), KeyError, r'vision_config\.patch_size'),
    (_edit('text_config', 'layer_norm_eps', None), KeyError, r'text_config\.layer_norm_eps'),
])
def test_refused_configurations_name_the_field(ref, tmp_path, edit, exc, names):
    with pytest.raises(exc, match=names):
        clip.load_clip(write_clip_dir(ref, 'a', tmp_path / 'd', config_edit=edit), 'cpu')


@pytest.mark.parametrize('key', ['vision_model.pre_layrnorm.weight', 'vision_model.encoder.layers.1.mlp.fc2.bias', 'visual_projection.weight',
                                 'vision_model.embeddings.class_embedding', 'text_model.encoder.layers.0.self_attn.k_proj.weight',
                                 'text_projection.weight'])
def test_missing_key_is_named(ref, tmp_path, key):
    with pytest.raises(KeyError, match=key.replace('.', r'\.')):
        clip.load_clip(write_clip_dir(ref, 'a', tmp_path / 'd', drop=(key,)), 'cpu')


def test_missing_files_and_wrong_shapes(ref, tmp_path):
    d = write_clip_dir(ref, 'a', tmp_path / 'd')
    os.remove(os.path.join(d, 'merges.txt'))
    with pytest.raises(FileNotFoundError, match='merges.txt'):
        clip.load_clip(d, 'cpu')
    # a position table of another image size: the configuration and the checkpoint disagree
    with pytest.raises(ValueError, match='position_embedding'):
        clip.load_clip(write_clip_dir(ref, 'a', tmp_path / 'e', config_edit=_edit('vision_config', 'image_size', 40)), 'cpu')


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_text_path_matches_the_golden(ref, tag, tmp_path):
    det = clip.load_clip(write_clip_dir(ref, tag, tmp_path / tag), 'cpu')
    ids0, ids1 = (torch.from_numpy(ref[f'{tag}/ids_{p}']) for p in ('pad0', 'padeos'))
    assert clip.first_eos(ids0, 63).tolist() == clip.first_eos(ids1, 63).tolist() == [3, 8, 15], 'pooled at the FIRST EOS'
    e0, e1 = det.text_embeds_from_ids(ids0), det.text_embeds_from_ids(ids1)
    assert e0.dtype == torch.float32 and e0.shape == (3, det.vision.cfg.projection_dim)
    # causal mask: whatever pads the row behind EOS cannot reach the pooled position (the embedding rows of the padding differ,
    # nothing else; the same fp32 arithmetic otherwise)
    torch.testing.assert_close(e0, e1, rtol=0, atol=1e-6)
    # fp32 torch against fp32 transformers, widths <= 96, 2 layers: the bound of the transformers.CLIPTextModel pin in
    # tests/test_host_logic.py (rtol 1e-4, atol 1e-5: ~100 fp32 roundings deep, values of order 1)
    torch.testing.assert_close(F.normalize(e1, dim=-1), torch.from_numpy(ref[f'{tag}/text_embeds']), rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError, match='EOS'):
        det.text_embeds_from_ids(torch.tensor([[62, 5, 6, 7]]))


@pytest.mark.parametrize('name,B,H,W,R,P', RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_fp64_restatement_is_the_reference_preprocessing(name, B, H, W, R, P):
    """The restatement the kernel is held to (tests/test_gpu_clip.py) is F.interpolate + normalise: a 16-term fp32 sum of values in
    [0, 1] with sum |w| <= 1.25^2, divided by std >= 0.26 -- within 1e-5 absolute of fp32 torch on the CPU."""
    img = case_images(name, B, H, W)
    x = F.interpolate(img.to(torch.float32) / 255., R, mode='bicubic', align_corners=False)
    x = (x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    got = pixel_values64(img, R)
    err = float((got - x.double()).abs().max())
    print(f'{name}: fp64 restatement vs F.interpolate fp32: {err:.2e}')
    assert err <= 1e-5
    if H == R and W == R:
        ident = (img.double() / 255 - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
        assert float((got - ident).abs().max()) <= 1e-15 * 8


def test_golden_pixel_values_are_the_restatement(ref):
    for tag in 'ab':
        R = json.loads(str(ref[f'{tag}/config']))['vision_config']['image_size']
        got = pixel_values64(torch.from_numpy(ref[f'{tag}/images']), R)
        assert float((got - torch.from_numpy(ref[f'{tag}/pixel_values']).double()).abs().max()) <= 1e-5


def test_load_detector_dispatch(ref, tmp_path):
    d = write_clip_dir(ref, 'a', tmp_path / 'a')
    assert metrics.is_clip_spec(d) and metrics.is_clip_spec('random:clip-tiny') and not metrics.is_clip_spec(str(tmp_path))
    det = metrics.load_detector(d, 'cpu')
    assert isinstance(det, clip.HipCLIPDetector) and not det.vision._ready, 'the compute copies are made at the first call'
    assert metrics.row_cosines(det) == det.scores
    fn = lambda *a, **k: 0                                                         # noqa: E731
    assert metrics.load_detector(fn, 'cpu') is fn
    # no GPU here: the image tower refuses instead of falling back
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
        det(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), texts=['a'])
    with pytest.raises(RuntimeError, match='no_grad'):
        det.vision(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
    for missing in (str(tmp_path / 'nope.pt'), str(tmp_path), None):
        with pytest.raises(FileNotFoundError) as e:
            metrics.load_detector(missing, 'cpu')
        assert str(e.value) == (f'feature detector {missing!r} not found: FID / CLIP metrics need the Inception / CLIP files the reference '
                                'downloads (metrics/sid_fid_and_clip.py:36, sid_metric_utils.py:456); pass a local file or a callable')


def test_row_cosines_of_a_plain_wrapper():
    f = F.normalize(torch.randn(4, 6, generator=torch.Generator().manual_seed(0)), dim=-1)
    wrapper = lambda images, texts, div255: torch.cat([f, f.flip(0)], 1)           # noqa: E731
    got = metrics.row_cosines(wrapper)(None, None)
    torch.testing.assert_close(got, (f * f.flip(0)).sum(-1))


def test_metric_clip_path_reaches_the_metric_options():
    import inspect
    from sid_lsg_amd.training_loop import evaluate_network, evaluate_teacher
    assert inspect.signature(metrics.MetricOptions).parameters['metric_clip_path'].default is None
    for fn in (evaluate_network, evaluate_teacher):
        assert inspect.signature(fn).parameters['metric_clip_path'].default is None
    opts = metrics.MetricOptions(G=None, prompts=['a'], device='cpu', metric_clip_path='random:clip-tiny')
    assert opts.metric_clip_path == 'random:clip-tiny' and opts.clip_score_fn is None


def test_sid_train_dry_run_unchanged(tmp_path, monkeypatch, golden_dir):
    from click.testing import CliRunner
    import sid_train
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a red cube\na blue sphere\n')
    monkeypatch.chdir(tmp_path)
    res = CliRunner().invoke(sid_train.main, [
        '--outdir', 'runs', '--data_prompt_text', '.', '--sd_model', 'random:tiny', '--seed', '3', '--batch', '8', '--batch-gpu', '2',
        '--duration', '0.01', '--ema', '0.05', '--cfg_train_fake', '1.5', '--cfg_eval_fake', '1.5', '--cfg_eval_real', '1.5', '--dry-run'])
    assert res.exit_code == 0, res.output
    with open(os.path.join(golden_dir, 'sid_train_dry_run.txt')) as f:
        assert res.output == f.read()
    helps = {f[0]: kw['help'] for f, kw in sid_train.OPTIONS if f[0] in ('--metric_clip_path', '--metric_open_clip_path')}
    assert all('compatibility' not in h and 'directory' in h for h in helps.values()) and len(helps) == 2


def test_golden_file_is_small_and_bf16_representable(ref, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, 'clip_ref.npz')) < 1_000_000
    for k in ref.files:
        if '/sd/' in k:
            w = torch.from_numpy(ref[k])
            assert torch.equal(w.to(torch.bfloat16).float(), w), k
    for tag in 'ab':
        np.testing.assert_allclose(ref[f'{tag}/cosines'], (ref[f'{tag}/image_embeds'] * ref[f'{tag}/text_embeds']).sum(-1), atol=1e-6)


def test_clip_score_tool_pairs_seeds_with_prompts(tmp_path):
    """tools/clip_score.py: <seed:06d>.png pairs with prompt line seed % len(prompts), generate_onestep.py's own pairing."""
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('clip_score_tool', os.path.join(root, 'tools', 'clip_score.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    (tmp_path / '000').mkdir()
    for name in ('000/000004.png', '000000.png', '000007.png', 'notes.txt', 'grid.png'):
        (tmp_path / name).write_bytes(b'')
    pairs = tool.paired_files(str(tmp_path), ['p0', 'p1', 'p2'])
    assert [(os.path.basename(p), t) for p, t in pairs] == [('000000.png', 'p0'), ('000004.png', 'p1'), ('000007.png', 'p1')]
    assert 'clip_score_tool' not in sys.modules
