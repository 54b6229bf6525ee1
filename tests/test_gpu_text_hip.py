"""The CLIP text encoder on the HIP kernels: sidlsg_attn_causal_fwd(_f32) and sidlsg_text_embed(_f32) against restatements,
text.HipCLIPTextModel against the torch module it replaces, and the seams that select it (load_sd15, TextConditioner, the samplers,
load_clip, the two command lines).

Measured on the MI355X (DESIGN.md carries the same numbers); worst per-sample relative l2 of the hidden states against the same state
dict in text.CLIPTextModel run in fp64 on the CPU, HipCLIPTextModel | the torch module on the same device at the same dtype:
  (i)   hidden 64, 2 layers, quick_gelu   fp32 1.018e-07 | 1.051e-07     bf16 4.132e-03 | 4.202e-03
  (ii)  hidden 128, 2 layers, gelu        fp32 1.273e-07 | 1.298e-07    bf16 4.261e-03 | 4.328e-03
  (iii) sd15 (12 layers, 768), batch 2    fp32 5.758e-07 | 3.811e-07   bf16 8.374e-03 | 8.541e-03
CLIP text tower (fp32 kernels) against the golden text_embeds of tests/golden/clip_ref.npz, worst relative l2 per row:
  (a) 1.10e-06, (b) 1.18e-06
"""
import copy
import glob
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from clip_ref_util import golden, write_clip_dir

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
# tests/test_gpu_ops.py::test_self_attention (bf16) and tests/test_gpu_fp32.py::test_self_attention_f32: max |err| <= tol * max |ref|
# against the fp64 attention of the same operands.  The mask adds no arithmetic.
ATTN_TOL = {BF16: 1.2e-2, F32: 2e-5}
# tests/test_gpu_clip.py: the bf16 image tower's |cosine - golden cosine|, asserted at 4x
TOWER_BF16_COS = {'a': 4.20e-3, 'b': 3.40e-3}
# measured on the MI355X (module docstring): the fp32 text tower's relative l2 against the golden text embeddings, asserted at 4x
TEXT_F32_REL_L2 = {'a': 1.10e-6, 'b': 1.18e-6}
SAMPLER_TOL = 3e-2            # tests/test_gpu_unet.py::test_glue_matches_reference_golden: bf16 UNet, relative to max |ref|


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


# ---- causal attention ------------------------------------------------------------------------------------------------------------
# The last three reach the padded widths, whose staging the causal kernels share with the two-set kernels (csrc/attn_short.h):
# (33, 40) D < DP in both dtypes, three waves, a ragged diagonal sub-tile; (17, 104) bf16 DP = 128 with 24 pad columns, fp32 DP = 112;
# (128, 128) the largest LDS image (72 KB bf16, 132 KB fp32), which launches only once the dynamic-LDS limit has been raised.
ATTN_SHAPES = [(2, 2, 77, 64), (1, 3, 77, 32), (2, 1, 1, 64), (1, 2, 16, 64), (1, 2, 17, 64), (1, 1, 128, 64),
               (1, 2, 33, 40), (1, 1, 17, 104), (1, 1, 128, 128)]


def _qkv(B, H, N, D, dtype):
    g = torch.Generator().manual_seed(1000 * N + D)
    return torch.randn(B, N, 3 * H * D, generator=g).to(dtype)


def causal_ref64(q, k, v, heads):
    """fp64 restatement: explicit -inf upper triangle, softmax, matmul."""
    B, N, C = q.shape
    d = C // heads
    qh, kh, vh = (t.double().reshape(B, N, heads, d).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * d ** -0.5
    s = s + torch.full((N, N), float('-inf'), dtype=F64).triu(1)
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, N, C)


@pytest.fixture(scope='module')
def attn_refs():
    """(shape, dtype) -> (qkv on the host, fp64 reference), computed once and left unchanged."""
    out = {}
    for shape in ATTN_SHAPES:
        B, H, N, D = shape
        C = H * D
        for dt in (BF16, F32):
            qkv = _qkv(B, H, N, D, dt)
            out[(shape, dt)] = (qkv, causal_ref64(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], H))
    return out


def _raw_causal(dtype, q, k, v, o, B, H, N, D, ldo=None, bso=None):
    from sid_lsg_amd import ops
    fn = ops._fn('attn_causal_fwd', dtype).raw
    ptr = lambda t: t if isinstance(t, int) else t.data_ptr()      # noqa: E731
    strides = [(t.stride(1), t.stride(0)) if torch.is_tensor(t) else (H * D, N * H * D) for t in (q, k, v)]
    return fn(ptr(q), ptr(k), ptr(v), ptr(o), B, H, N, D, strides[0][0], strides[1][0], strides[2][0], ldo or H * D, strides[0][1],
              strides[1][1], strides[2][1], bso or N * H * D, ops._s())


def _check_attn(got, want, dtype, name):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f'{name}: every element of rows < N is written and finite'
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f'{name}: max |err| {err:.3e} = {err / scale:.3e} of max |ref| (bound {ATTN_TOL[dtype]:g})')
    assert err <= ATTN_TOL[dtype] * scale


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('shape', ATTN_SHAPES, ids=['x'.join(map(str, s)) for s in ATTN_SHAPES])
def test_causal_attention(dev, attn_refs, shape, dtype):
    from sid_lsg_amd import ops
    B, H, N, D = shape
    C = H * D
    qkv, want = attn_refs[(shape, dtype)]
    d_qkv = qkv.to(dev)
    # (1) the fused [B, N, 3C] buffer in place, through the raw entry point into a NaN-filled output
    out = torch.full((B, N, C), float('nan'), device=dev, dtype=dtype)
    q, k, v = d_qkv[..., :C], d_qkv[..., C:2 * C], d_qkv[..., 2 * C:]
    assert _raw_causal(dtype, q, k, v, out, B, H, N, D) == 0
    _check_attn(out, want, dtype, f'{shape} fused')
    assert torch.equal(ops.causal_self_attention(d_qkv, H), out), 'the public wrapper is the same launch'
    # (2) three separate tensors whose batch stride is larger than N * C (and an output view with a larger batch stride too)
    pad = 24
    bufs = [torch.full((B, N + 1, C + pad), float('nan'), device=dev, dtype=dtype) for _ in range(3)]
    views = []
    for buf, src in zip(bufs, (q, k, v)):
        buf[:, :N, :C] = src
        views.append(buf[:, :N, :C])
    assert all(t.stride(0) > N * C and t.stride(1) == C + pad for t in views)
    got = ops.causal_attention(*views, H)
    _check_attn(got, want, dtype, f'{shape} separate')
    obuf = torch.full((B, N + 3, C), float('nan'), device=dev, dtype=dtype)
    assert _raw_causal(dtype, *views, obuf, B, H, N, D, bso=(N + 3) * C) == 0
    assert torch.equal(obuf[:, :N], got)
    assert torch.isnan(obuf[:, N:]).all(), 'query rows >= N are never stored'


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
def test_causality_bit_for_bit(dev, attn_refs, dtype):
    """Keys and values at positions >= p replaced by large finite values (not NaN: 0 x NaN in the PV product is NaN in any flash
    kernel): rows < p keep their bits, rows >= p change."""
    from sid_lsg_amd import ops
    B, H, N, D = shape = (2, 2, 77, 64)
    C = H * D
    d_qkv = attn_refs[(shape, dtype)][0].to(dev)
    first = ops.causal_self_attention(d_qkv, H)
    sign = torch.where(torch.arange(2 * C, device=dev) % 2 == 0, 1e4, -1e4).to(dtype)
    for p in (1, 16, 17, 76):
        mod = d_qkv.clone()
        mod[:, p:, C:] = sign
        out = ops.causal_self_attention(mod, H)
        assert torch.isfinite(out.float()).all()
        assert torch.equal(out[:, :p], first[:, :p]), f'p = {p}: rows < p saw a key >= p'
        differs = (out[:, p:] != first[:, p:]).flatten(2).any(2)
        assert bool(differs.all()), f'p = {p}: a row >= p did not change'


def test_causal_attention_refusals(dev):
    from sid_lsg_amd import ops
    for dtype in (BF16, F32):
        big = torch.zeros(1, 129, 3 * 64, device=dev, dtype=dtype)
        out = torch.zeros(1, 129, 64, device=dev, dtype=dtype)
        q, k, v = big[..., :64], big[..., 64:128], big[..., 128:]
        assert _raw_causal(dtype, q, k, v, out, 1, 1, 129, 64) == EINVAL
        assert _raw_causal(dtype, q, k, v, out, 1, 1, 0, 64) == EINVAL
        assert _raw_causal(dtype, q, k, v, out, 1, 1, 16, 12) == EINVAL
        assert _raw_causal(dtype, q.data_ptr() + big.element_size(), k, v, out, 1, 1, 16, 64) == EINVAL, 'misaligned Q'
        assert _raw_causal(dtype, q, k, v, out.data_ptr() + out.element_size(), 1, 1, 16, 64) == EINVAL, 'misaligned O'
        assert _raw_causal(dtype, q, k, v, out, 1, 1, 16, 64) == 0
        with pytest.raises(RuntimeError, match='1 <= N <= 128'):
            ops.causal_self_attention(big, 1)
        with pytest.raises(RuntimeError, match='1 <= N <= 128'):
            ops.causal_self_attention(big[:, :0], 1)
        with pytest.raises(RuntimeError, match='multiple of 8'):
            ops.causal_self_attention(torch.zeros(1, 16, 36, device=dev, dtype=dtype), 1)
        with pytest.raises(RuntimeError, match='sidlsg_attn_causal_fwd(_f32)? failed with code -22'):
            flat = torch.zeros(16 * 192 + 8, device=dev, dtype=dtype)
            ops.causal_self_attention(flat[1:1 + 16 * 192].view(1, 16, 192), 1)
        with pytest.raises(RuntimeError, match='forward only'):
            ops.causal_self_attention(big[:, :16].clone().requires_grad_(), 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.causal_self_attention(torch.zeros(1, 16, 192), 1)


# ---- text_embed ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,D,V', [(3, 77, 64, 1000), (1, 77, 768, 49408)])
def test_text_embed(dev, B, L, D, V):
    from sid_lsg_amd import ops
    g = torch.Generator().manual_seed(V)
    tok, pos = torch.randn(V, D, generator=g), torch.randn(L + 3, D, generator=g)
    ids = torch.randint(0, V, (B, L), generator=g)
    ids[0, 0], ids[-1, -1] = 0, V - 1
    want = tok[ids] + pos[:L]
    d_tok, d_pos = tok.to(dev), pos.to(dev)
    for d_ids in (ids.to(dev), ids):            # device ids, and host ids (checked and copied by the wrapper)
        got = ops.text_embed(d_ids, d_tok, d_pos, F32)
        assert got.dtype == F32 and got.shape == (B * L, D)
        assert torch.equal(got.cpu().view(B, L, D), want)
        assert torch.equal(ops.text_embed(d_ids, d_tok, d_pos, BF16).cpu().view(B, L, D), want.to(BF16))
    bad = ids.clone()
    bad[0, 1], bad[-1, 5] = V, -1
    for dt in (F32, BF16):
        got = ops.text_embed(bad.to(dev), d_tok, d_pos, dt).cpu().view(B, L, D)
        nan_rows = torch.isnan(got.float()).all(-1)
        assert torch.equal(nan_rows, (bad < 0) | (bad >= V)), 'all-NaN rows exactly at the ids outside [0, V)'
        assert torch.equal(got[~nan_rows], want.to(dt)[~nan_rows])
    with pytest.raises(ValueError, match=f'token id {V} is outside'):
        ops.text_embed(bad, d_tok, d_pos, F32)
    with pytest.raises(RuntimeError, match='position embeddings'):
        ops.text_embed(torch.zeros(1, L + 4, dtype=torch.long, device=dev), d_tok, d_pos)
    with pytest.raises(RuntimeError, match='multiple of 8'):
        ops.text_embed(ids.to(dev), d_tok[:, :12].contiguous(), d_pos[:, :12].contiguous())


# ---- the encoder against the module it replaces ----------------------------------------------------------------------------------
ENCODERS = {'i': dict(hidden=64, layers=2, heads=2, dff=128, act='quick_gelu'), 'ii': dict(hidden=128, layers=2, heads=2, dff=256, act='gelu')}
PROMPTS = ['', 'a red cube', 'word ' * 90]            # the empty prompt, a short one, one longer than 77 tokens (truncated)


def _encoder_case(name):
    from sid_lsg_amd.text import TEXT_CONFIGS, CLIPTextModel, HashTokenizer
    cfg = TEXT_CONFIGS['sd15'] if name == 'iii' else ENCODERS[name]
    torch.manual_seed({'i': 11, 'ii': 12, 'iii': 13}[name])
    enc = CLIPTextModel(**cfg).requires_grad_(False).eval()
    ids = HashTokenizer()(PROMPTS[1:] if name == 'iii' else PROMPTS).input_ids
    assert ids.shape == ((2 if name == 'iii' else 3), 77) and int(ids[-1, -1]) == 49407 and int(ids[-1, -2]) != 49407, 'the long prompt was truncated'
    return cfg, enc, ids


def _rel_l2(got, want):
    got, want = got.double().cpu(), want.double()
    return float(((got - want).flatten(1).norm(dim=1) / want.flatten(1).norm(dim=1)).max())


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', ['i', 'ii', 'iii'])
def test_encoder_matches_the_torch_module(dev, name, dtype):
    """Reference: the same state dict in text.CLIPTextModel, fp64 on the CPU.  Bound: the error of the torch module on the same device
    at the same dtype -- the thing being replaced -- times 2: the two differ in accumulation order and in where they round (fused
    q|k|v, residual in the GEMM epilogue), not in precision class."""
    from sid_lsg_amd.text import CLIPTextModel, HipCLIPTextModel
    cfg, enc, ids = _encoder_case(name)
    torch_enc = enc.to(dtype).to(dev)
    state = {k: v.detach().cpu() for k, v in torch_enc.state_dict().items()}
    ref = CLIPTextModel(**cfg).double().requires_grad_(False).eval()
    ref.load_state_dict({k: v.double() for k, v in state.items()})
    with torch.no_grad():
        want = ref(ids)[0]
        base = torch_enc(ids.to(dev))[0]
    hip = HipCLIPTextModel.from_torch(copy.deepcopy(torch_enc))
    got = hip(ids.to(dev))[0]
    assert got.dtype == dtype and got.shape == want.shape and torch.isfinite(got.float()).all()
    e_hip, e_torch = _rel_l2(got, want), _rel_l2(base, want)
    print(f'encoder ({name}) {dtype}: worst per-sample relative l2 against fp64: HIP {e_hip:.3e}, torch module on the device {e_torch:.3e}')
    assert e_hip <= 2 * e_torch


@pytest.mark.parametrize('p', [1, 17])
def test_encoder_level_causality(dev, p):
    from sid_lsg_amd.text import HipCLIPTextModel
    cfg, enc, ids = _encoder_case('i')
    hip = HipCLIPTextModel.from_torch(enc).to(BF16).to(dev)
    g = torch.Generator().manual_seed(p)
    row = torch.randint(0, 49406, (77,), generator=g)
    other = row.clone()
    other[p:] = (row[p:] + 1 + torch.randint(0, 1000, (77 - p,), generator=g)) % 49406
    assert torch.equal(row[:p], other[:p]) and bool((row[p:] != other[p:]).all())
    h = hip(torch.stack([row, other]).to(dev))[0]
    assert torch.equal(h[0, :p], h[1, :p]), 'hidden states before p depend on tokens from p on'
    assert not torch.equal(h[0, p], h[1, p])


# ---- duck-typing -----------------------------------------------------------------------------------------------------------------
def test_load_sd15_returns_the_hip_module_with_the_same_weights(dev, monkeypatch):
    from sid_lsg_amd.sd_util import load_sd15
    from sid_lsg_amd.text import CLIPTextModel, HipCLIPTextModel
    monkeypatch.delenv('SIDLSG_TEXT_ENCODER', raising=False)
    out_h = load_sd15('random:tiny', None, dev, F32, text_encoder='hip')
    out_t = load_sd15('random:tiny', None, dev, F32, text_encoder='torch')
    assert len(out_h) == len(out_t) == 5
    hip, te, tok = out_h[3], out_t[3], out_h[4]
    assert type(hip) is HipCLIPTextModel and type(te) is CLIPTextModel and type(load_sd15('random:tiny', None, dev, F32)[3]) is CLIPTextModel
    sh, st = hip.state_dict(), te.state_dict()
    assert list(sh) == list(st) and all(torch.equal(sh[k], st[k]) for k in st)
    assert hip.device.type == 'cuda' and hip.dtype == F32 and hip.config.hidden_size == te.config.hidden_size
    ids = tok(['a red cube', '']).input_ids.to(dev)
    h32 = hip(ids)[0]
    assert h32.dtype == F32 and h32.shape == (2, tok.model_max_length, hip.config.hidden_size)
    hip = hip.to(BF16)
    h16 = hip(ids)[0]
    assert h16.dtype == BF16 and not torch.equal(h16.float(), h32), 'the bf16 kernels took over: the compute copies were rebuilt'
    for clone in (copy.deepcopy(hip), pickle.loads(pickle.dumps(hip))):
        assert type(clone) is HipCLIPTextModel and torch.equal(clone(ids)[0], h16)
    new = {k: (v + 0.25 if k.endswith('final_layer_norm.bias') else v) for k, v in hip.state_dict().items()}
    hip.load_state_dict(new)
    moved = hip(ids)[0]
    assert not torch.equal(moved, h16), 'load_state_dict dropped the compute copies'
    assert float((moved.float() - h16.float() - 0.25).abs().max()) <= 2 ** -6 * float(moved.float().abs().max())
    with pytest.raises(ValueError, match='attention_mask'):
        hip(ids, attention_mask=torch.ones_like(ids))


# ---- through the seams -----------------------------------------------------------------------------------------------------------
def _sample(unet, vae, sched, te, tok, dev):
    from sid_lsg_amd.sd_util import sid_sd_sampler
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        return sid_sd_sampler(unet=unet, latents=z, contexts=['a red cube', 'two dogs on a hill'], init_timesteps=torch.full((2,), 625, device=dev),
                              noise_scheduler=sched, text_encoder=te, tokenizer=tok, resolution=64, dtype=F32, return_images=True, vae=vae,
                              train_sampler=False)


@pytest.mark.parametrize('how', ['argument', 'environment'])
def test_sampler_with_the_hip_encoder(dev, monkeypatch, how):
    from sid_lsg_amd.sd_util import load_sd15
    from sid_lsg_amd.text import HipCLIPTextModel, TextConditioner
    monkeypatch.delenv('SIDLSG_TEXT_ENCODER', raising=False)
    unet, vae, sched, te, tok = load_sd15('random:tiny', None, dev, BF16)
    unet.eval().requires_grad_(False)
    if how == 'argument':
        hip = load_sd15('random:tiny', None, dev, BF16, text_encoder='hip')[3]
    else:
        monkeypatch.setenv('SIDLSG_TEXT_ENCODER', 'hip')
        hip = load_sd15('random:tiny', None, dev, BF16)[3]
    assert type(hip) is HipCLIPTextModel
    cond = TextConditioner(tok, hip)
    c, u = cond.encode(['a red cube', 'two dogs on a hill']), cond.uncond(2)
    assert c.dtype == BF16 and c.shape == u.shape == (2, tok.model_max_length, hip.config.hidden_size) and c.is_contiguous()
    assert torch.equal(u[0], u[1]) and torch.equal(u[0], cond.encode([''])[0])
    want, got = _sample(unet, vae, sched, te, tok, dev), _sample(unet, vae, sched, hip, tok, dev)
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = float((got - want).abs().max() / want.abs().max())
    print(f'sid_sd_sampler on random:tiny, HIP against torch text encoder ({how}): max |diff| / max |ref| = {err:.3e}')
    assert err <= SAMPLER_TOL


# ---- CLIP score ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def clip_dirs(golden_dir, tmp_path_factory):
    ref = golden(golden_dir)
    root = tmp_path_factory.mktemp('clip_text')
    return ref, {tag: write_clip_dir(ref, tag, root / tag) for tag in 'ab'}


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_clip_score_with_the_hip_text_tower(dev, clip_dirs, tag):
    """The golden carries token ids, not strings: the text half is taken from them, as tests/test_gpu_clip.py does.  Head widths 16
    (a) and 24 (b) over 16 tokens: the padded tiling of the fp32 causal kernel.  bf16 image tower: the golden cosines within 4x the
    figure tests/test_gpu_clip.py records; fp32: the text embeddings within 4x the relative l2 measured on the MI355X."""
    from sid_lsg_amd import ops
    from sid_lsg_amd.clip import load_clip
    from sid_lsg_amd.text import HipCLIPTextModel
    ref, dirs = clip_dirs
    images, ids = torch.from_numpy(ref[f'{tag}/images']).to(dev), torch.from_numpy(ref[f'{tag}/ids_padeos'])
    det = load_clip(dirs[tag], dev, text_tower='hip')
    assert type(det.text_encoder) is HipCLIPTextModel
    with torch.no_grad():
        feats, cos = ops.clip_score(det.vision(images), det.text_embeds_from_ids(ids).contiguous())
    err = (cos.cpu().double() - torch.from_numpy(ref[f'{tag}/cosines']).double()).abs()
    print(f'clip ({tag}) bf16 image tower, HIP text tower: |cosine - golden| {err.tolist()}')
    assert float(err.max()) <= 4 * TOWER_BF16_COS[tag]
    texts = ['a cat', 'two dogs on a hill', 'x']
    s = det.scores(images, texts)
    s_torch = load_clip(dirs[tag], dev).scores(images, texts)
    # both text towers are fp32 arithmetic on 16 tokens of a 2-layer network: their normalised embeddings differ in the last few fp32
    # ulps, and a cosine (a 24- or 32-term dot product of unit vectors) by no more than a few times 1e-7
    assert s.shape == (3,) and float((s - s_torch).abs().max()) <= 1e-5, 'the same scores as with the torch text tower, from strings'
    got = feats[:, feats.shape[1] // 2:].cpu().double()
    want = torch.from_numpy(ref[f'{tag}/text_embeds']).double()
    rel = (got - want).norm(dim=-1) / want.norm(dim=-1)
    print(f'clip ({tag}) fp32 HIP text tower: relative l2 per row against the golden text_embeds {rel.tolist()}')
    assert float(rel.max()) <= 4 * TEXT_F32_REL_L2[tag]


# ---- command lines ---------------------------------------------------------------------------------------------------------------
def _run(args, timeout):
    with socket.socket() as sock:           # a rendezvous port of the child's own: this process may hold the default one
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, MASTER_PORT=str(port))
    env.pop('SIDLSG_TEXT_ENCODER', None)
    res = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def test_generate_onestep_with_the_hip_encoder(dev, tmp_path):
    prompts = tmp_path / 'prompts.txt'
    prompts.write_text('a red cube\na blue sphere\n')
    out = tmp_path / 'img'
    log = _run([os.path.join(ROOT, 'generate_onestep.py'), '--network', 'teacher', '--teacher_steps', '2', '--guidance_scale', '2', '--outdir', str(out),
                '--seeds', '0-1', '--text_prompts', str(prompts), '--repo_id', 'random:tiny', '--resolution', '64', '--text_encoder', 'hip'], 240)
    files = sorted(glob.glob(str(out / '*.png')))
    assert [os.path.basename(f) for f in files] == ['000000.png', '000001.png'], log
    import PIL.Image
    img = np.asarray(PIL.Image.open(files[0]).convert('RGB'))
    assert img.shape == (64, 64, 3) and img.min() != img.max()


def test_sid_train_with_the_hip_encoder(dev, tmp_path):
    """One tick (1 kimg = 32 iterations of 32 images at 64 x 64) of `sid_train.py --text_encoder hip` on random:tiny."""
    import json
    (tmp_path / 'aesthetics_6_plus.txt').write_text('\n'.join(f'prompt number {i}' for i in range(40)) + '\n')
    runs = tmp_path / 'runs'
    _run([os.path.join(ROOT, 'sid_train.py'), '--outdir', str(runs), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny', '--seed', '1',
          '--batch', '32', '--batch-gpu', '32', '--duration', '0.000002', '--ema', '0.00001', '--tick', '1', '--snap', '50', '--dump', '50',
          '--resolution', '64', '--text_encoder', 'hip'], 240)
    run_dir = glob.glob(str(runs / '00000-*'))[0]
    assert json.load(open(os.path.join(run_dir, 'training_options.json')))['text_encoder'] == 'hip'
    stats = glob.glob(os.path.join(run_dir, 'stats_*.jsonl'))
    assert stats and os.path.getsize(stats[0]) > 0
