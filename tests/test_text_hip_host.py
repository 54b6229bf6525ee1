"""The HIP text encoder, host side (no GPU): the option surface (sid_train.py / generate_onestep.py / load_sd15 / load_clip), the module's
duck-typing of text.CLIPTextModel, its refusals, and the header declarations of the four new entry points."""
import copy
import json
import pickle

import pytest
import torch

TINY = dict(hidden=64, layers=2, heads=2, dff=128, vocab=1000, max_pos=13, act='quick_gelu')


def _dry_run(tmp_path, *extra):
    from click.testing import CliRunner
    import sid_train
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a red cube\na blue sphere\n')
    return CliRunner().invoke(sid_train.main, [
        '--outdir', str(tmp_path / 'runs'), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny', '--seed', '3', '--batch', '8',
        '--batch-gpu', '2', '--duration', '0.01', '--dry-run', *extra])


@pytest.mark.parametrize('kind', ['hip', 'torch'])
def test_sid_train_dry_run_shows_the_text_encoder(tmp_path, kind):
    res = _dry_run(tmp_path, '--text_encoder', kind)
    assert res.exit_code == 0, res.output
    opts = json.loads(res.output[res.output.index('{'):res.output.rindex('}') + 1])
    assert opts['text_encoder'] == kind


def test_sid_train_text_encoder_is_absent_unless_given_and_refuses_other_values(tmp_path):
    res = _dry_run(tmp_path)
    assert res.exit_code == 0, res.output
    assert '"text_encoder"' not in res.output, 'the printed options of a run without the option stay as they were'
    bad = _dry_run(tmp_path, '--text_encoder', 'cuda')
    assert bad.exit_code != 0 and "'cuda' is not one of" in bad.output, bad.output


def test_the_option_reaches_every_load_sd15_call_of_the_loop(monkeypatch, tmp_path):
    """training, --train_mode 0 and the teacher row: each forwards text_encoder to load_sd15, and passes nothing when it was not given."""
    from sid_lsg_amd import training_loop as tl
    seen = []

    class Stop(Exception):
        pass

    def factory(**kw):
        seen.append(kw.get('text_encoder', 'absent'))
        raise Stop
    monkeypatch.setattr(tl, 'load_sd15', factory)
    snap = tmp_path / 'network-snapshot-000001.pkl'
    snap.write_bytes(b'x')
    common = dict(run_dir=str(tmp_path), device=torch.device('cpu'), pretrained_model_name_or_path='random:tiny', metrics=['fid_test'],
                  dataset_prompt_text_kwargs=dict(class_name='sid_lsg_amd.data.PromptDataset', path=str(tmp_path), resolution=64, prompt_only=True))
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a red cube\na blue sphere\n')
    for mode in (dict(train_mode=True, batch_size=2), dict(train_mode=False, network_pkl=str(snap)), dict(train_mode=False, network_pkl='teacher')):
        for kind in ('hip', None):
            with pytest.raises(Stop):
                tl.training_loop(**common, **mode, **({} if kind is None else dict(text_encoder=kind)))
    assert seen == ['hip', 'absent'] * 3


def test_generate_onestep_help_and_choice(tmp_path):
    from click.testing import CliRunner
    import generate_onestep as g
    res = CliRunner().invoke(g.main, ['--help'])
    text = ' '.join(res.output.split())            # click wraps the help text
    assert res.exit_code == 0 and '--text_encoder [torch|hip]' in text and 'HIP kernels [default: $SIDLSG_TEXT_ENCODER, else torch] (not a reference option)' in text
    bad = CliRunner().invoke(g.main, ['--network', 'teacher', '--outdir', str(tmp_path), '--repo_id', 'random:tiny', '--text_encoder', 'cuda'])
    assert bad.exit_code != 0 and "'cuda' is not one of" in bad.output, bad.output


def test_state_dict_keys_and_strict_load():
    from sid_lsg_amd.text import CLIPTextModel, HipCLIPTextModel
    torch.manual_seed(0)
    ref = CLIPTextModel(**TINY)
    hip = HipCLIPTextModel(**TINY)
    assert isinstance(hip, CLIPTextModel)
    assert list(hip.state_dict()) == list(ref.state_dict())
    res = hip.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(a, b) for a, b in zip(hip.state_dict().values(), ref.state_dict().values()))
    # from_torch shares the parameters of the module it wraps, and leaves the class of an already converted one alone
    wrapped = HipCLIPTextModel.from_torch(ref)
    assert type(wrapped) is HipCLIPTextModel and HipCLIPTextModel.from_torch(wrapped) is wrapped
    assert all(a is b for a, b in zip(wrapped.parameters(), ref.parameters()))
    assert wrapped.config is ref.config and wrapped.dtype == torch.float32 and wrapped.device.type == 'cpu'
    for clone in (copy.deepcopy(wrapped), pickle.loads(pickle.dumps(wrapped))):
        assert type(clone) is HipCLIPTextModel and clone._hip_cache is None
        assert all(torch.equal(a, b) for a, b in zip(clone.state_dict().values(), ref.state_dict().values()))
    assert wrapped.to(torch.bfloat16).dtype == torch.bfloat16
    with pytest.raises(TypeError):
        HipCLIPTextModel.from_torch(torch.nn.Linear(2, 2))


def test_refusals_on_the_host():
    from sid_lsg_amd.text import HipCLIPTextModel
    hip = HipCLIPTextModel(**TINY)
    ids = torch.zeros(2, 13, dtype=torch.long)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip(ids)
    with pytest.raises(ValueError, match='attention_mask'):
        hip(ids, attention_mask=torch.ones(2, 13))


def test_load_sd15_and_load_clip_refuse_unknown_kinds(monkeypatch):
    from sid_lsg_amd import clip, sd_util
    from sid_lsg_amd.text import resolve_text_encoder
    with pytest.raises(ValueError, match="'cuda'"):
        sd_util.load_sd15('random:tiny', None, 'cpu', torch.float32, text_encoder='cuda')
    with pytest.raises(ValueError, match="'cuda'"):
        clip.load_clip('random:clip-tiny', 'cpu', text_tower='cuda')
    monkeypatch.delenv('SIDLSG_TEXT_ENCODER', raising=False)
    assert resolve_text_encoder() == 'torch' and resolve_text_encoder('hip') == 'hip'
    monkeypatch.setenv('SIDLSG_TEXT_ENCODER', 'hip')
    assert resolve_text_encoder() == 'hip' and resolve_text_encoder('torch') == 'torch', 'the argument wins over the environment'
    monkeypatch.setenv('SIDLSG_TEXT_ENCODER', 'rocm')
    with pytest.raises(ValueError, match="'rocm'"):
        resolve_text_encoder()


def test_load_clip_text_tower_on_the_host():
    from sid_lsg_amd import clip
    from sid_lsg_amd.text import CLIPTextModel, HipCLIPTextModel
    a, b = clip.load_clip('random:clip-tiny', 'cpu'), clip.load_clip('random:clip-tiny', 'cpu', text_tower='hip')
    assert type(a.text_encoder) is CLIPTextModel and type(b.text_encoder) is HipCLIPTextModel
    sa, sb = a.text_encoder.state_dict(), b.text_encoder.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_entry_points_are_declared_in_the_header():
    import ctypes
    from sid_lsg_amd._lib import parse_header
    protos = parse_header()
    attn = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 8 + [ctypes.c_longlong] * 4 + [ctypes.c_void_p]
    embed = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    for name, args in (('sidlsg_attn_causal_fwd', attn), ('sidlsg_attn_causal_fwd_f32', attn), ('sidlsg_text_embed', embed),
                       ('sidlsg_text_embed_f32', embed)):
        assert protos.get(name) == args, name
