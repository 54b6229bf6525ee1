"""CLIP score from a local CLIP directory: the ViT image tower on the HIP kernels, the text tower in PyTorch or on them.

Reference: networks/clip.py (the open_clip wrapper the metrics un-pickle: `forward(images, texts, div255)` -> the L2-normalised
`image | text` features, :48-53; preprocessing :33-37) and metrics/sid_metric_utils.py:456-504 (the mean cosine of the two
halves is the CLIP score).  The wrapper needs open_clip, timm and torchvision; this module needs a directory in the Hugging
Face layout instead (`openai/clip-vit-large-patch14`, `laion/CLIP-ViT-g-14-laion2B-s12B-b42K`, ...):

    config.json          vision_config / text_config / projection_dim
    model.safetensors    the transformers key names (vision_model.*, visual_projection.weight, text_model.*, text_projection.weight)
    vocab.json merges.txt

  * `HipCLIPVisionTower`: transformers' CLIPVisionModelWithProjection arithmetic on this package's kernels -- preprocessing and
    patch extraction in one launch (ops.clip_patches), ONE GEMM for patch embedding + class token + position embeddings (the
    latter two through its `res` operand), pre-LN layers on ops.layer_norm / ops.gemm / ops.self_attention / ops.gelu, the final
    LayerNorm and projection on the class token only.  Frozen, inference only.
  * the text side is `text.CLIPTextModel` (PyTorch; the default) or, with load_clip(..., text_tower='hip'), the same weights as
    `text.HipCLIPTextModel` on the HIP kernels; either way pooled at the first EOS token and projected.
  * `HipCLIPDetector`: the wrapper's call contract, finished by ops.clip_score (normalise both, concatenate, cosine).
  * `load_clip('random:clip-<arch>')`: seeded random networks with the hash tokenizer, for timing and tests (no weights offline).
  * `load_open_clip(checkpoint, tokenizer_dir)`: the same towers from a checkpoint in open_clip's own layout (HPS_v2_compressed.pt,
    open_clip_pytorch_model.bin), behind open_clip's validation transform: `HipCLIPVisionTower(..., preprocess='pil')` swaps the
    float interpolation for Pillow's 8-bit BICUBIC resize + centre crop (ops.pil_patches, one launch, bit-equal to Pillow).
There is no fallback: the image tower runs on the GPU kernels or raises.
"""
import json
import os
from types import SimpleNamespace

import torch

from . import ops
from .text import TEXT_ENCODERS, CLIPBPETokenizer, CLIPTextModel, HashTokenizer, HipCLIPTextModel

BF16, F32 = torch.bfloat16, torch.float32

VISION_FIELDS = ('hidden_size', 'intermediate_size', 'num_hidden_layers', 'num_attention_heads', 'image_size', 'patch_size',
                 'hidden_act', 'layer_norm_eps')
TEXT_FIELDS = ('hidden_size', 'intermediate_size', 'num_hidden_layers', 'num_attention_heads', 'hidden_act', 'layer_norm_eps')
ACTS = ('quick_gelu', 'gelu')
MAX_TEXT_LEN = 77

_V = dict(hidden_act='quick_gelu', layer_norm_eps=1e-5, image_size=224, patch_size=14)
_T = dict(hidden_act='quick_gelu', layer_norm_eps=1e-5, vocab_size=49408, max_position_embeddings=77, eos_token_id=49407)
CLIP_ARCHS = {
    'tiny': dict(projection_dim=32,
                 vision_config=dict(_V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=32, patch_size=8),
                 text_config=dict(_T, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2)),
    'vit-l-14': dict(projection_dim=768,            # openai/clip-vit-large-patch14
                     vision_config=dict(_V, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16),
                     text_config=dict(_T, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12)),
    'vit-l-14-336': dict(projection_dim=768,        # openai/clip-vit-large-patch14-336, the image tower of the published CMMD
                         vision_config=dict(_V, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=336),
                         text_config=dict(_T, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12)),
    'vit-g-14': dict(projection_dim=1024,           # laion/CLIP-ViT-g-14-laion2B-s12B-b42K (what the reference's clip_score.py builds)
                     vision_config=dict(_V, hidden_size=1408, intermediate_size=6144, num_hidden_layers=40, num_attention_heads=16, hidden_act='gelu'),
                     text_config=dict(_T, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, hidden_act='gelu')),
    'vit-h-14': dict(projection_dim=1024,           # laion/CLIP-ViT-H-14-laion2B-s32B-b79K, the model HPSv2 fine-tunes (head dim 80)
                     vision_config=dict(_V, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, hidden_act='gelu'),
                     text_config=dict(_T, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, hidden_act='gelu')),
}
PREPROCESS = ('interpolate', 'pil')      # ops.clip_patches (the reference's CLIP-score wrapper) / ops.pil_patches (open_clip's validation transform)
# What a state dict in open_clip's layout does not say: head counts and the activation (widths are there to be checked against the shapes)
OPEN_CLIP_ARCHS = {
    'tiny': dict(vision_width=64, vision_heads=2, text_width=64, text_heads=2, act='gelu'),
    'ViT-L-14': dict(vision_width=1024, vision_heads=16, text_width=768, text_heads=12, act='gelu'),
    'ViT-H-14': dict(vision_width=1280, vision_heads=16, text_width=1024, text_heads=16, act='gelu'),
    'ViT-g-14': dict(vision_width=1408, vision_heads=16, text_width=1024, text_heads=16, act='gelu'),
}


def parse_clip_config(cfg, where='config.json'):
    """The fields of a transformers CLIPConfig dict this module reproduces -> (vision, text) namespaces; raises, naming the item,
    on a missing field or a configuration the kernels would not reproduce."""
    for part, fields in (('vision_config', VISION_FIELDS), ('text_config', TEXT_FIELDS)):
        if not isinstance(cfg.get(part), dict):
            raise KeyError(f'{where}: {part} is missing')
        for f in fields:
            if f not in cfg[part]:
                raise KeyError(f'{where}: {part}.{f} is missing')
    if 'projection_dim' not in cfg:
        raise KeyError(f'{where}: projection_dim is missing')
    v = SimpleNamespace(**{f: cfg['vision_config'][f] for f in VISION_FIELDS}, projection_dim=int(cfg['projection_dim']))
    tc = cfg['text_config']
    t = SimpleNamespace(**{f: tc[f] for f in TEXT_FIELDS}, projection_dim=int(cfg['projection_dim']), vocab_size=int(tc.get('vocab_size', 49408)),
                        max_position_embeddings=int(tc.get('max_position_embeddings', 77)), eos_token_id=int(tc.get('eos_token_id', 49407)))
    if t.eos_token_id == 2:
        # early transformers CLIP configs carry eos_token_id 2 and pool at argmax(ids): with CLIP's vocabulary that is the first
        # occurrence of the highest id, <|endoftext|>
        t.eos_token_id = t.vocab_size - 1
    for part, c in (('vision_config', v), ('text_config', t)):
        if c.hidden_act not in ACTS:
            raise ValueError(f'{where}: {part}.hidden_act = {c.hidden_act!r}: only {ACTS} are implemented')
        if c.hidden_size % c.num_attention_heads:
            raise ValueError(f'{where}: {part}.num_attention_heads = {c.num_attention_heads} does not divide hidden_size = {c.hidden_size}')
    head = v.hidden_size // v.num_attention_heads
    if head % 8 or head > 160:
        raise ValueError(f'{where}: vision_config.num_attention_heads = {v.num_attention_heads} gives head dim {head}: the attention kernel '
                         'takes multiples of 8 up to 160')
    if v.image_size % v.patch_size:
        raise ValueError(f'{where}: vision_config.image_size % patch_size != 0 ({v.image_size} % {v.patch_size})')
    if v.hidden_size % 8 or v.hidden_size > 2048 or v.intermediate_size % 8 or v.projection_dim <= 0:
        raise ValueError(f'{where}: vision_config.hidden_size = {v.hidden_size} / intermediate_size = {v.intermediate_size}: the LayerNorm '
                         'and GEMM kernels take multiples of 8, hidden_size <= 2048')
    return v, t


def vision_keys(cfg):
    """Every key of the image tower, transformers' names."""
    keys = ['vision_model.embeddings.patch_embedding.weight', 'vision_model.embeddings.class_embedding',
            'vision_model.embeddings.position_embedding.weight', 'visual_projection.weight']
    for ln in ('pre_layrnorm', 'post_layernorm'):            # `pre_layrnorm` is transformers' spelling
        keys += [f'vision_model.{ln}.weight', f'vision_model.{ln}.bias']
    for i in range(cfg.num_hidden_layers):
        p = f'vision_model.encoder.layers.{i}.'
        for m in ('self_attn.q_proj', 'self_attn.k_proj', 'self_attn.v_proj', 'self_attn.out_proj', 'layer_norm1', 'layer_norm2', 'mlp.fc1', 'mlp.fc2'):
            keys += [p + m + '.weight', p + m + '.bias']
    return keys


class HipCLIPVisionTower:
    """transformers' CLIPVisionModelWithProjection on the HIP kernels: uint8 images -> [B, projection_dim] fp32 image embeddings
    (not yet normalised).  `state`: fp32 masters under the transformers key names; the compute copies are bf16 (default) or, with
    compute_dtype=torch.float32, fp32 (the `_f32` kernel family, as HipUNet2DCondition).  Frozen: runs under no_grad only."""

    def __init__(self, cfg, state, device, compute_dtype=None, preprocess='interpolate'):
        self.cfg = cfg
        self.device = torch.device(device)
        self.compute_dtype = compute_dtype or BF16
        if self.compute_dtype not in (BF16, F32):
            raise ValueError(f'compute_dtype {compute_dtype}: expected torch.bfloat16 or torch.float32')
        if preprocess not in PREPROCESS:
            raise ValueError(f'preprocess {preprocess!r}: expected one of {PREPROCESS}')
        self.preprocess = preprocess
        self.grid = cfg.image_size // cfg.patch_size
        self.tokens = 1 + self.grid ** 2
        self.masters = {}
        for k in vision_keys(cfg):
            if k not in state:
                raise KeyError(f'CLIP image tower: {k} is missing from the checkpoint')
            self.masters[k] = state[k].detach().to(self.device, F32).contiguous()
        C, P = cfg.hidden_size, cfg.patch_size
        shapes = {'vision_model.embeddings.patch_embedding.weight': (C, 3, P, P), 'vision_model.embeddings.class_embedding': (C,),
                  'vision_model.embeddings.position_embedding.weight': (self.tokens, C), 'visual_projection.weight': (cfg.projection_dim, C),
                  'vision_model.encoder.layers.0.mlp.fc1.weight': (cfg.intermediate_size, C)}
        for k, s in shapes.items():
            if tuple(self.masters[k].shape) != s:
                raise ValueError(f'CLIP image tower: {k} has shape {tuple(self.masters[k].shape)}, the configuration says {s}')
        self._ready = False
        self._res = {}

    def _prepare(self):
        m, cd, cfg = self.masters, self.compute_dtype, self.cfg
        C, kp = cfg.hidden_size, ops.clip_patch_width(cfg.patch_size)
        w = torch.zeros((C, kp), device=self.device, dtype=F32)
        w[:, :3 * cfg.patch_size ** 2] = m['vision_model.embeddings.patch_embedding.weight'].reshape(C, -1)
        self.w_patch = w.to(cd)
        pos = m['vision_model.embeddings.position_embedding.weight'].clone()
        pos[0] += m['vision_model.embeddings.class_embedding']
        self.pos = pos.to(cd)                                             # [T, C]: position embeddings, class embedding in row 0
        self.ln_pre = (m['vision_model.pre_layrnorm.weight'], m['vision_model.pre_layrnorm.bias'])
        self.ln_post = (m['vision_model.post_layernorm.weight'], m['vision_model.post_layernorm.bias'])
        self.w_proj = m['visual_projection.weight'].to(cd)
        self.layers = []
        for i in range(cfg.num_hidden_layers):
            p = f'vision_model.encoder.layers.{i}.'
            qkv = [p + f'self_attn.{n}_proj' for n in 'qkv']
            self.layers.append(SimpleNamespace(
                ln1=(m[p + 'layer_norm1.weight'], m[p + 'layer_norm1.bias']), ln2=(m[p + 'layer_norm2.weight'], m[p + 'layer_norm2.bias']),
                w_qkv=torch.cat([m[k + '.weight'] for k in qkv]).to(cd), b_qkv=torch.cat([m[k + '.bias'] for k in qkv]),
                w_o=m[p + 'self_attn.out_proj.weight'].to(cd), b_o=m[p + 'self_attn.out_proj.bias'],
                w_1=m[p + 'mlp.fc1.weight'].to(cd), b_1=m[p + 'mlp.fc1.bias'], w_2=m[p + 'mlp.fc2.weight'].to(cd), b_2=m[p + 'mlp.fc2.bias']))
        self._ready = True

    def _check(self, images_u8):
        if torch.is_grad_enabled():
            raise RuntimeError('HipCLIPVisionTower is frozen and forward only: call it under torch.no_grad()')
        if images_u8.device.type != 'cuda':
            raise RuntimeError('HipCLIPVisionTower runs on the MI355X only (no CPU fallback)')
        if images_u8.dtype != torch.uint8:
            raise RuntimeError(f'HipCLIPVisionTower takes uint8 images, got {images_u8.dtype}')
        if not self._ready:
            self._prepare()

    def embed(self, images_u8):
        """uint8 [B, 3, H, W] -> the token tensor [B * T, C] in front of pre_layrnorm: patch embeddings + position embeddings, the
        class embedding in row 0 of every image -- one ops.clip_patches (preprocess='pil': ops.pil_patches) launch and one GEMM."""
        self._check(images_u8)
        B = images_u8.shape[0]
        if B not in self._res:
            self._res = {B: self.pos.repeat(B, 1)}                       # the cached res operand of the current batch size
        patches = ops.pil_patches if self.preprocess == 'pil' else ops.clip_patches
        a = patches(images_u8.contiguous(), self.cfg.image_size, self.cfg.patch_size, self.compute_dtype)
        return ops.gemm(a, self.w_patch, res=self._res[B])

    def __call__(self, images_u8):
        cfg = self.cfg
        x = self.embed(images_u8)
        B, T, C, eps = images_u8.shape[0], self.tokens, cfg.hidden_size, float(cfg.layer_norm_eps)
        x = ops.layer_norm(x, *self.ln_pre, eps)
        for lyr in self.layers:
            qkv = ops.gemm(ops.layer_norm(x, *lyr.ln1, eps), lyr.w_qkv, bias=lyr.b_qkv)
            o = ops.self_attention(qkv.view(B, T, 3 * C), cfg.num_attention_heads)
            x = ops.gemm(o.view(B * T, C), lyr.w_o, bias=lyr.b_o, res=x)
            h = ops.gelu(ops.gemm(ops.layer_norm(x, *lyr.ln2, eps), lyr.w_1, bias=lyr.b_1), cfg.hidden_act)
            x = ops.gemm(h, lyr.w_2, bias=lyr.b_2, res=x)
        cls = ops.layer_norm(x.view(B, T, C)[:, 0].contiguous(), *self.ln_post, eps)
        return ops.gemm(cls, self.w_proj, out_f32=True)


def first_eos(ids, eos_token_id):
    """[B] position of the first EOS token of every row (transformers' pooling position)."""
    hit = ids == eos_token_id
    if not bool(hit.any(1).all()):
        raise ValueError(f'token ids without the EOS token {eos_token_id}: nothing to pool the text embedding at')
    return hit.int().argmax(1)


class HipCLIPDetector:
    """The reference wrapper's contract (networks/clip.py:48-53): `det(images_u8, texts=[...], div255=True)` -> [B, 2F] fp32, the
    L2-normalised image | text embeddings; `det.scores(images_u8, texts)` -> [B] cosines (what the metrics average)."""

    def __init__(self, vision, text_encoder, text_projection, tokenizer, eos_token_id):
        self.vision, self.text_encoder, self.tokenizer, self.eos_token_id = vision, text_encoder, tokenizer, eos_token_id
        self.text_projection = text_projection                            # [F, hidden] fp32
        self.device = vision.device

    @property
    def preprocess(self):
        """'interpolate' or 'pil': the image preprocessing of the tower (HipCLIPVisionTower)."""
        return self.vision.preprocess

    @torch.no_grad()
    def text_embeds_from_ids(self, ids):
        """[B, L] token ids -> [B, F] fp32 (not normalised): the last layer's states after final_layer_norm, pooled at the first EOS
        and projected.  The mask is causal, so whatever pads the row after EOS cannot change the result."""
        ids = ids.to(self.text_projection.device)
        h = self.text_encoder(ids)[0].float()
        pooled = h[torch.arange(ids.shape[0], device=ids.device), first_eos(ids, self.eos_token_id)]
        return pooled @ self.text_projection.t()

    def encode_text(self, texts):
        tok = self.tokenizer
        return self.text_embeds_from_ids(tok(list(texts), padding='max_length', max_length=tok.model_max_length, truncation=True,
                                             return_tensors='pt').input_ids)

    @torch.no_grad()
    def _features(self, images, texts, div255=True):
        if not div255:
            raise ValueError('HipCLIPDetector takes uint8 images (div255=True): the preprocessing kernel divides by 255 itself')
        if texts is None or len(texts) != len(images):
            raise ValueError('HipCLIPDetector: one text per image')
        return ops.clip_score(self.vision(images).contiguous(), self.encode_text(texts).contiguous())

    def __call__(self, images, texts=None, div255=True):
        return self._features(images, texts, div255)[0]

    def scores(self, images, texts):
        return self._features(images, texts)[1]


def _text_tower(t, device):
    enc = CLIPTextModel(hidden=t.hidden_size, layers=t.num_hidden_layers, heads=t.num_attention_heads, dff=t.intermediate_size,
                        vocab=t.vocab_size, max_pos=t.max_position_embeddings, act=t.hidden_act)
    for mod in enc.modules():
        if isinstance(mod, torch.nn.LayerNorm):
            mod.eps = float(t.layer_norm_eps)
    return enc


def _random_state(v, t, device, seed):
    """Seeded random weights under the transformers key names (normal, std 0.02 / fan-in scaled; norms = identity)."""
    g = torch.Generator(device=device).manual_seed(seed)
    C = v.hidden_size
    rnd = lambda *s, std: torch.randn(*s, device=device, generator=g) * std      # noqa: E731
    sd = {'vision_model.embeddings.patch_embedding.weight': rnd(C, 3, v.patch_size, v.patch_size, std=(3 * v.patch_size ** 2) ** -0.5),
          'vision_model.embeddings.class_embedding': rnd(C, std=0.5),
          'vision_model.embeddings.position_embedding.weight': rnd(1 + (v.image_size // v.patch_size) ** 2, C, std=0.5),
          'visual_projection.weight': rnd(v.projection_dim, C, std=C ** -0.5),
          'text_projection.weight': rnd(t.projection_dim, t.hidden_size, std=t.hidden_size ** -0.5)}
    for k in vision_keys(v):
        if k in sd:
            continue
        if 'norm' in k:
            sd[k] = torch.ones(C, device=device) if k.endswith('weight') else torch.zeros(C, device=device)
        elif k.endswith('bias'):
            sd[k] = rnd(v.intermediate_size if 'fc1' in k else C, std=0.02)
        else:
            n, kk = (v.intermediate_size, C) if 'fc1' in k else ((C, v.intermediate_size) if 'fc2' in k else (C, C))
            sd[k] = rnd(n, kk, std=kk ** -0.5)
    return sd


def load_clip(path, device, compute_dtype=None, seed=0, text_tower='torch', preprocess='interpolate'):
    """A HipCLIPDetector from a local directory in the Hugging Face layout (module docstring), or from 'random:clip-<arch>'
    (CLIP_ARCHS; seeded weights, hash tokenizer).  text_tower: 'torch' (text.CLIPTextModel) or 'hip' (text.HipCLIPTextModel, the same
    fp32 weights on the fp32 kernel family).  preprocess: 'interpolate' (the reference's CLIP-score wrapper) or 'pil' (open_clip's
    validation transform, ops.pil_patches)."""
    if text_tower not in TEXT_ENCODERS:
        raise ValueError(f'text_tower {text_tower!r}: expected one of {TEXT_ENCODERS}')
    device = torch.device(device)
    name = str(path)
    if name.lower().startswith('random:'):
        arch = name.lower()[len('random:'):]
        if not arch.startswith('clip-') or arch[5:] not in CLIP_ARCHS:
            raise ValueError(f"{name}: expected 'random:clip-<arch>' with <arch> in {sorted(CLIP_ARCHS)}")
        v, t = parse_clip_config(CLIP_ARCHS[arch[5:]], name)
        state = _random_state(v, t, device, seed)
        rng = torch.random.get_rng_state()
        torch.manual_seed(seed + 1)
        text = _text_tower(t, device)
        torch.random.set_rng_state(rng)
        tokenizer = HashTokenizer(model_max_length=min(MAX_TEXT_LEN, t.max_position_embeddings))
    else:
        cj = os.path.join(name, 'config.json')
        if not os.path.isfile(cj):
            raise FileNotFoundError(f'{name}: not a CLIP directory (no config.json)')
        with open(cj) as f:
            v, t = parse_clip_config(json.load(f), cj)
        st = os.path.join(name, 'model.safetensors')
        if not os.path.isfile(st):
            raise FileNotFoundError(f'{st}: the weights of the CLIP directory are missing')
        from safetensors.torch import load_file
        state = load_file(st)
        text = _text_tower(t, device)
        want = dict(text.state_dict())
        for k in list(want) + ['text_projection.weight']:
            if k not in state:
                raise KeyError(f'{st}: {k} is missing from the checkpoint')
        for k, w in want.items():
            if tuple(state[k].shape) != tuple(w.shape):
                raise ValueError(f'{st}: {k} has shape {tuple(state[k].shape)}, the configuration says {tuple(w.shape)}')
        text.load_state_dict({k: state[k].float() for k in want})
        vj, mt = os.path.join(name, 'vocab.json'), os.path.join(name, 'merges.txt')
        for p in (vj, mt):
            if not os.path.isfile(p):
                raise FileNotFoundError(f'{p}: the tokenizer files of the CLIP directory are missing')
        tokenizer = CLIPBPETokenizer.from_files(vj, mt, model_max_length=min(MAX_TEXT_LEN, t.max_position_embeddings), pad_token_id=t.eos_token_id)
        for attr, word in (('bos_token_id', '<|startoftext|>'), ('eos_token_id', '<|endoftext|>')):
            if word not in tokenizer.vocab:
                raise KeyError(f'{vj}: {word} is missing from the vocabulary')
            setattr(tokenizer, attr, tokenizer.vocab[word])
        if tokenizer.eos_token_id != t.eos_token_id:
            raise ValueError(f'{cj}: text_config.eos_token_id = {t.eos_token_id}, but {vj} has <|endoftext|> = {tokenizer.eos_token_id}')
    vision = HipCLIPVisionTower(v, state, device, compute_dtype, preprocess)
    text = text.float().requires_grad_(False).eval().to(device)
    if text_tower == 'hip':
        text = HipCLIPTextModel.from_torch(text)
    return HipCLIPDetector(vision, text, state['text_projection.weight'].detach().to(device, F32), tokenizer, t.eos_token_id)


def parse_vision_config(cfg, where='config.json'):
    """The image tower's fields from either a full CLIP config (`vision_config` + `projection_dim`) or the flat
    CLIPVisionModelWithProjection config (the fields at top level) -> the vision namespace, checked as parse_clip_config checks it."""
    vc = cfg['vision_config'] if isinstance(cfg.get('vision_config'), dict) else cfg
    part = 'vision_config' if vc is not cfg else 'config'
    for f in VISION_FIELDS:
        if f not in vc:
            raise KeyError(f'{where}: {part}.{f} is missing')
    pd = cfg.get('projection_dim', vc.get('projection_dim'))
    if pd is None:
        raise KeyError(f'{where}: projection_dim is missing')
    t = dict(hidden_size=8, intermediate_size=8, num_hidden_layers=1, num_attention_heads=1, hidden_act=ACTS[0], layer_norm_eps=1e-5)
    return parse_clip_config(dict(vision_config={f: vc[f] for f in VISION_FIELDS}, text_config=t, projection_dim=int(pd)), where)[0]


def load_clip_vision(path, device, compute_dtype=None, seed=0, preprocess='pil'):
    """The image tower alone (HipCLIPVisionTower; an IP-Adapter's image encoder): a local directory with config.json (full CLIP config or
    the flat CLIPVisionModelWithProjection one) and model.safetensors, of which only the vision_keys are required, or
    'random:clip-<arch>' (the seeded image tower load_clip builds for that spec)."""
    device = torch.device(device)
    name = str(path)
    if name.lower().startswith('random:'):
        arch = name.lower()[len('random:'):]
        if not arch.startswith('clip-') or arch[5:] not in CLIP_ARCHS:
            raise ValueError(f"{name}: expected 'random:clip-<arch>' with <arch> in {sorted(CLIP_ARCHS)}")
        v, t = parse_clip_config(CLIP_ARCHS[arch[5:]], name)
        return HipCLIPVisionTower(v, _random_state(v, t, device, seed), device, compute_dtype, preprocess)
    cj, st = os.path.join(name, 'config.json'), os.path.join(name, 'model.safetensors')
    if not os.path.isfile(cj):
        raise FileNotFoundError(f'{name}: not a CLIP image encoder directory (no config.json)')
    if not os.path.isfile(st):
        raise FileNotFoundError(f'{st}: the weights of the CLIP image encoder directory are missing')
    with open(cj) as f:
        v = parse_vision_config(json.load(f), cj)
    from safetensors.torch import load_file
    return HipCLIPVisionTower(v, load_file(st), device, compute_dtype, preprocess)


# ---- checkpoints in open_clip's layout (HPS_v2_compressed.pt, open_clip_pytorch_model.bin, open_clip_model.safetensors) ---------------
_OC_LAYER = (('ln_1', 'layer_norm1'), ('ln_2', 'layer_norm2'), ('attn.out_proj', 'self_attn.out_proj'), ('mlp.c_fc', 'mlp.fc1'),
             ('mlp.c_proj', 'mlp.fc2'))


def open_clip_state(obj):
    """What torch.load / load_file returned -> the flat state dict: the `state_dict` entry when there is one, a leading `module.`
    (DistributedDataParallel) stripped."""
    if isinstance(obj, dict) and isinstance(obj.get('state_dict'), dict):
        obj = obj['state_dict']
    if not isinstance(obj, dict):
        raise ValueError(f'open_clip checkpoint: expected a state dict, got {type(obj).__name__}')
    return {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in obj.items()}


def open_clip_to_transformers(state, arch='ViT-H-14', where='open_clip checkpoint'):
    """A state dict under open_clip's names -> (the same tensors under the transformers names the towers take, the config dict
    parse_clip_config reads).  in_proj_{weight,bias} are split into q / k / v rows, visual.proj and text_projection transposed,
    logit_scale and attn_mask dropped.  Widths, depth, patch and image size come from the shapes; head counts and the activation
    from OPEN_CLIP_ARCHS[arch].  Raises, naming the key, on a missing key, and, naming the item, where shapes and table disagree."""
    if arch not in OPEN_CLIP_ARCHS:
        raise ValueError(f'arch {arch!r}: expected one of {sorted(OPEN_CLIP_ARCHS)}')
    tab = OPEN_CLIP_ARCHS[arch]
    state = open_clip_state(state)

    def get(k, ndim=None):
        if k not in state:
            raise KeyError(f'{where}: {k} is missing')
        t = state[k].detach().float()
        if ndim is not None and t.dim() != ndim:
            raise ValueError(f'{where}: {k} has shape {tuple(t.shape)}: expected {ndim} dimensions')
        return t
    out = {}
    conv = get('visual.conv1.weight', 4)
    C, P = conv.shape[0], conv.shape[2]
    if C != tab['vision_width']:
        raise ValueError(f'{where}: visual.conv1.weight has {C} output channels, arch {arch} has vision width {tab["vision_width"]}')
    pos = get('visual.positional_embedding', 2)
    grid = int(round((pos.shape[0] - 1) ** 0.5))
    if grid * grid + 1 != pos.shape[0]:
        raise ValueError(f'{where}: visual.positional_embedding has {pos.shape[0]} rows: not 1 + a square grid')
    vproj, tproj = get('visual.proj', 2), get('text_projection', 2)
    tok, tpos = get('token_embedding.weight', 2), get('positional_embedding', 2)
    D = tok.shape[1]
    if D != tab['text_width']:
        raise ValueError(f'{where}: token_embedding.weight has width {D}, arch {arch} has text width {tab["text_width"]}')
    if vproj.shape[1] != tproj.shape[1]:
        raise ValueError(f'{where}: visual.proj projects to {vproj.shape[1]}, text_projection to {tproj.shape[1]}')
    out['vision_model.embeddings.patch_embedding.weight'] = conv
    out['vision_model.embeddings.class_embedding'] = get('visual.class_embedding', 1)
    out['vision_model.embeddings.position_embedding.weight'] = pos
    out['visual_projection.weight'] = vproj.t().contiguous()
    out['text_projection.weight'] = tproj.t().contiguous()
    out['text_model.embeddings.token_embedding.weight'] = tok
    out['text_model.embeddings.position_embedding.weight'] = tpos
    for oc, hf in (('visual.ln_pre', 'vision_model.pre_layrnorm'), ('visual.ln_post', 'vision_model.post_layernorm'),
                   ('ln_final', 'text_model.final_layer_norm')):
        for p in ('weight', 'bias'):
            out[f'{hf}.{p}'] = get(f'{oc}.{p}', 1)
    depth, dff = {}, {}
    for side, src, dst, width in (('vision', 'visual.transformer.resblocks.', 'vision_model.encoder.layers.', C),
                                  ('text', 'transformer.resblocks.', 'text_model.encoder.layers.', D)):
        n = 0
        while f'{src}{n}.attn.in_proj_weight' in state:
            w, b = get(f'{src}{n}.attn.in_proj_weight', 2), get(f'{src}{n}.attn.in_proj_bias', 1)
            if tuple(w.shape) != (3 * width, width) or tuple(b.shape) != (3 * width,):
                raise ValueError(f'{where}: {src}{n}.attn.in_proj_weight / bias have shapes {tuple(w.shape)} / {tuple(b.shape)}, the width '
                                 f'{width} says {(3 * width, width)} / {(3 * width,)}')
            for j, name in enumerate('qkv'):
                out[f'{dst}{n}.self_attn.{name}_proj.weight'] = w[j * width:(j + 1) * width].contiguous()
                out[f'{dst}{n}.self_attn.{name}_proj.bias'] = b[j * width:(j + 1) * width].contiguous()
            for oc, hf in _OC_LAYER:
                for p in ('weight', 'bias'):
                    out[f'{dst}{n}.{hf}.{p}'] = get(f'{src}{n}.{oc}.{p}')
            n += 1
        if n == 0:
            raise KeyError(f'{where}: {src}0.attn.in_proj_weight is missing')
        depth[side], dff[side] = n, out[f'{dst}0.mlp.fc1.weight'].shape[0]
    for side, width in (('vision', C), ('text', D)):
        if width % tab[f'{side}_heads']:
            raise ValueError(f'{where}: arch {arch} has {tab[f"{side}_heads"]} {side} heads, which do not divide the width {width}')
    cfg = dict(projection_dim=int(vproj.shape[1]),
               vision_config=dict(hidden_size=C, intermediate_size=dff['vision'], num_hidden_layers=depth['vision'],
                                  num_attention_heads=tab['vision_heads'], image_size=grid * P, patch_size=P, hidden_act=tab['act'],
                                  layer_norm_eps=1e-5),
               text_config=dict(hidden_size=D, intermediate_size=dff['text'], num_hidden_layers=depth['text'],
                                num_attention_heads=tab['text_heads'], hidden_act=tab['act'], layer_norm_eps=1e-5, vocab_size=int(tok.shape[0]),
                                max_position_embeddings=int(tpos.shape[0]), eos_token_id=int(tok.shape[0]) - 1))
    return out, cfg


def load_open_clip(checkpoint, tokenizer_dir, device, arch='ViT-H-14', compute_dtype=None, text_tower='torch', preprocess='pil'):
    """A HipCLIPDetector from a checkpoint in open_clip's layout: `.pt` / `.bin` (torch.load(weights_only=True)) or `.safetensors`,
    flat or under a `state_dict` entry (HPS_v2_compressed.pt, open_clip_pytorch_model.bin of the LAION repositories), mapped by
    open_clip_to_transformers.  The tokenizer is CLIPBPETokenizer on vocab.json / merges.txt of `tokenizer_dir` (the tokenizer/
    directory of any Stable Diffusion model has the vocabulary).  The image preprocessing is open_clip's validation transform
    (preprocess='pil') unless asked otherwise."""
    if text_tower not in TEXT_ENCODERS:
        raise ValueError(f'text_tower {text_tower!r}: expected one of {TEXT_ENCODERS}')
    name = str(checkpoint)
    if not os.path.isfile(name):
        raise FileNotFoundError(f'{name}: the open_clip checkpoint is missing')
    if name.endswith('.safetensors'):
        from safetensors.torch import load_file
        raw = load_file(name)
    else:
        raw = torch.load(name, map_location='cpu', weights_only=True)
    state, cfg = open_clip_to_transformers(raw, arch, name)
    v, t = parse_clip_config(cfg, f'{name} (arch {arch})')
    text = _text_tower(t, device)
    want = dict(text.state_dict())
    for k, w in want.items():
        if k not in state:
            raise KeyError(f'{name}: no tensor maps to {k}')
        if tuple(state[k].shape) != tuple(w.shape):
            raise ValueError(f'{name}: {k} has shape {tuple(state[k].shape)}, the configuration says {tuple(w.shape)}')
    text.load_state_dict({k: state[k].float() for k in want})
    vj, mt = os.path.join(str(tokenizer_dir), 'vocab.json'), os.path.join(str(tokenizer_dir), 'merges.txt')
    for p in (vj, mt):
        if not os.path.isfile(p):
            raise FileNotFoundError(f'{p}: the tokenizer files are missing')
    tokenizer = CLIPBPETokenizer.from_files(vj, mt, model_max_length=min(MAX_TEXT_LEN, t.max_position_embeddings), pad_token_id=t.eos_token_id)
    for attr, word in (('bos_token_id', '<|startoftext|>'), ('eos_token_id', '<|endoftext|>')):
        if word not in tokenizer.vocab:
            raise KeyError(f'{vj}: {word} is missing from the vocabulary')
        setattr(tokenizer, attr, tokenizer.vocab[word])
    if tokenizer.eos_token_id != t.eos_token_id or max(tokenizer.vocab.values()) >= t.vocab_size:
        raise ValueError(f'{vj}: <|endoftext|> = {tokenizer.eos_token_id} and {max(tokenizer.vocab.values()) + 1} entries, but {name} embeds '
                         f'{t.vocab_size} tokens (the last one is <|endoftext|>)')
    vision = HipCLIPVisionTower(v, state, device, compute_dtype, preprocess)
    text = text.float().requires_grad_(False).eval().to(device)
    if text_tower == 'hip':
        text = HipCLIPTextModel.from_torch(text)
    return HipCLIPDetector(vision, text, state['text_projection.weight'].detach().to(device, F32), tokenizer, t.eos_token_id)
