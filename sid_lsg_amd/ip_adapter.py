"""IP-Adapter (Ye et al. 2023) image prompts on the HIP kernels, forward only: the SD 1.5 adapters with the linear image projection.

A reference picture becomes T image tokens (T = 4 in the published SD 1.5 adapters); every cross-attention layer of the UNet runs a
second attention over them with the layer's own queries and adds it, scaled, to its text attention ("decoupled cross-attention"):

    attn2(x) = to_out( softmax(q K^T) V  +  s * softmax(q K2^T) V2 ),   K2 = to_k_ip(tokens), V2 = to_v_ip(tokens)

  * `image_proj`: tokens = LayerNorm(reshape(Linear(image_embeds), [T, Dctx])) -- one GEMM with bias and one LayerNorm;
  * all layers' `to_k_ip | to_v_ip` compute weights live in ONE concatenated [sum 2 C_l, Dctx] matrix: HipIPAdapter.prepare runs ONE GEMM
    per batch and layer l reads its K2 | V2 as a column slice of the result -- nothing of the adapter runs inside a sampling loop
    except the attention itself;
  * the attention is ONE launch per layer (ops.cross_attention2, csrc/ip_attn.hip) in place of the text attention's: no second
    attention launch, no add, one rounding.
A guided [uncond ; cond] batch (dup = 2) gives its unconditional half the projection of ZERO image embeddings: bias and LayerNorm still
act, as in the published pipeline.

The module rules, the checkpoint key names, the layer numbering (`ip_adapter.<2 i + 1>`, i counting the cross-attention layers in the
order of diffusers' `attn_processors`: down blocks, up blocks, mid block) and the unconditional rule restate the published IP-Adapter
code and diffusers' loader from memory; neither is installed here, so agreement with them is not pinned by a test
(tests/ip_adapter_ref.py is a torch.nn restatement of the same rules).
"""
import os

import torch

from . import ops
from .unet import BF16, F32

RANDOM_PREFIX = 'random:ip-adapter'
RANDOM_TOKENS = 4
MAX_TOKENS = ops.CROSS2_MAX_KEYS2
LN_EPS = 1e-5
PROJ_KEYS = ('image_proj.proj.weight', 'image_proj.proj.bias', 'image_proj.norm.weight', 'image_proj.norm.bias')


def layer_table(cfg):
    """THE mapping of checkpoint layer numbers to cross-attention layers: [(n, where, C_l)] with n = 2 i + 1 and i counting the UNet's
    attn2 modules in the order of HipUNet2DCondition.cross_attention_layers (down_blocks, up_blocks, mid_block).  SD 1.5: 1, 3, ..., 31,
    the mid block at 31."""
    ch, L = cfg.block_out_channels, cfg.layers_per_block
    rows = []
    for i, c in enumerate(ch):
        if cfg.down_has_attn[i]:
            rows += [(f'down_blocks.{i}.attentions.{j}', c) for j in range(L)]
    for i, (c, has) in enumerate(zip(reversed(ch), reversed(cfg.down_has_attn))):
        if has:
            rows += [(f'up_blocks.{i}.attentions.{j}', c) for j in range(L + 1)]
    rows.append(('mid_block.attentions.0', ch[-1]))
    return [(2 * i + 1, where, c) for i, (where, c) in enumerate(rows)]


def expected_keys(cfg):
    keys = list(PROJ_KEYS)
    for n, _, _ in layer_table(cfg):
        keys += [f'ip_adapter.{n}.to_k_ip.weight', f'ip_adapter.{n}.to_v_ip.weight']
    return keys


def parse_random_spec(spec):
    """'random:ip-adapter' -> None (the caller's seed), 'random:ip-adapter:<seed>' -> the seed; any other 'random:...' is a ValueError."""
    parts = str(spec).lower().split(':')
    if parts[:2] != RANDOM_PREFIX.split(':') or len(parts) > 3:
        raise ValueError(f"{spec}: expected '{RANDOM_PREFIX}' or '{RANDOM_PREFIX}:<seed>'")
    if len(parts) == 2:
        return None
    if not parts[2].isdigit():
        raise ValueError(f'{spec}: the seed must be a non-negative integer')
    return int(parts[2])


def random_state_dict(cfg, embed_dim, seed=0, tokens=RANDOM_TOKENS):
    """Seeded fan-in-scaled NON-zero weights under the published key names (CPU fp32): an adapter that changes the UNet's output."""
    g = torch.Generator().manual_seed(int(seed))
    dctx = cfg.cross_attention_dim
    sd = {'image_proj.proj.weight': torch.randn(tokens * dctx, embed_dim, generator=g) * embed_dim ** -0.5,
          'image_proj.proj.bias': torch.randn(tokens * dctx, generator=g) * 0.5,
          'image_proj.norm.weight': 1 + 0.1 * torch.randn(dctx, generator=g),
          'image_proj.norm.bias': 0.1 * torch.randn(dctx, generator=g)}
    for n, _, c in layer_table(cfg):
        sd[f'ip_adapter.{n}.to_k_ip.weight'] = torch.randn(c, dctx, generator=g) * dctx ** -0.5
        sd[f'ip_adapter.{n}.to_v_ip.weight'] = torch.randn(c, dctx, generator=g) * dctx ** -0.5
    return sd


def flatten_state(obj, where='IP-Adapter checkpoint'):
    """The nested form of a `.bin` ({'image_proj': {...}, 'ip_adapter': {...}}) -> the flat keys of the `.safetensors` form; a flat dict
    passes through."""
    if not isinstance(obj, dict):
        raise ValueError(f'{where}: expected a dict of tensors, got {type(obj).__name__}')
    if any(isinstance(v, dict) for v in obj.values()):
        flat = {}
        for top, sub in obj.items():
            if not isinstance(sub, dict):
                raise ValueError(f'{where}: unexpected key {top} next to nested entries')
            for k, v in sub.items():
                flat[f'{top}.{k}'] = v
        return flat
    return dict(obj)


def check_state_dict(sd, cfg, embed_dim=None, where='IP-Adapter checkpoint'):
    """Every key and shape of a flat state dict against the UNet configuration -> T.  Refuses by name: Resampler keys (the "plus" and
    FaceID families), a missing or unexpected key, a wrong shape (which is also what the other plausible layer order -- mid block before
    the up blocks -- produces), T > 32, and an embedding width different from `embed_dim`."""
    for k in sd:
        if k.startswith('image_proj.') and k not in PROJ_KEYS:
            raise ValueError(f'{where}: {k}: a Resampler / "plus" / FaceID image projection is not supported (only the linear projection '
                             'image_proj.proj + image_proj.norm)')
    want = expected_keys(cfg)
    for k in want:
        if k not in sd:
            raise ValueError(f'{where}: missing key {k}')
    extra = sorted(set(sd) - set(want))
    if extra:
        raise ValueError(f'{where}: unexpected key {extra[0]}' + (f' (and {len(extra) - 1} more)' if len(extra) > 1 else ''))
    dctx = cfg.cross_attention_dim
    pw = sd['image_proj.proj.weight']
    if pw.dim() != 2 or pw.shape[0] % dctx or pw.shape[0] == 0:
        raise ValueError(f'{where}: image_proj.proj.weight has shape {tuple(pw.shape)}: expected [T * {dctx}, E] (cross_attention_dim {dctx})')
    T, E = pw.shape[0] // dctx, pw.shape[1]
    if T > MAX_TOKENS:
        raise ValueError(f'{where}: image_proj.proj.weight gives T = {T} image tokens: at most {MAX_TOKENS} are supported')
    if embed_dim is not None and E != embed_dim:
        raise ValueError(f'{where}: image_proj.proj.weight takes embeddings of width E = {E}, the image encoder has projection_dim {embed_dim}')
    shapes = {'image_proj.proj.bias': (T * dctx,), 'image_proj.norm.weight': (dctx,), 'image_proj.norm.bias': (dctx,)}
    for n, where_l, c in layer_table(cfg):
        shapes[f'ip_adapter.{n}.to_k_ip.weight'] = shapes[f'ip_adapter.{n}.to_v_ip.weight'] = (c, dctx)
    for k, s in shapes.items():
        if tuple(sd[k].shape) != s:
            raise ValueError(f'{where}: {k} has shape {tuple(sd[k].shape)}, expected {s} (layer numbers follow down blocks, up blocks, mid '
                             'block; a file in another order is refused, not guessed)')
    return T


def read_state_file(path):
    """A local `.safetensors` (flat keys) or `.bin` (nested, torch.load(weights_only=True)) -> flat state dict."""
    name = str(path)
    if not os.path.isfile(name):
        raise FileNotFoundError(f"{name}: not a local IP-Adapter file; pass a .safetensors / .bin file or '{RANDOM_PREFIX}[:seed]'")
    if name.lower().endswith('.safetensors'):
        from safetensors.torch import load_file
        return flatten_state(load_file(name), name)
    if name.lower().endswith('.bin'):
        return flatten_state(torch.load(name, map_location='cpu', weights_only=True), name)
    raise ValueError(f'{name}: expected a .safetensors or .bin file')


def nested_state(sd):
    """The flat keys -> the nested form a `.bin` holds."""
    out = {'image_proj': {}, 'ip_adapter': {}}
    for k, v in sd.items():
        top, rest = k.split('.', 1)
        out[top][rest] = v
    return out


class IPState:
    """What a sampling loop carries: the wide K2 | V2 buffer [B, T, sum 2 C_l] of one batch (computed once), the scale and the column
    offsets of the layers.  Made by HipIPAdapter.prepare; consumed by HipUNet2DCondition.forward_nhwc(ip=...)."""

    def __init__(self, adapter, tokens, kv, scale):
        self.adapter, self.tokens, self.kv, self.scale = adapter, tokens, kv, float(scale)

    def layer_kv(self, i):
        """[B, T, 2 C_i]: the column slice of layer i (K2 in the first C_i columns, V2 in the rest)."""
        off, c = self.adapter.offsets[i], self.adapter.channels[i]
        return self.kv[:, :, off:off + 2 * c]

    def bind(self, unet, x, ctx):
        """The checks of an image-prompt pass, then every attn2 of `unet` gets its (K2 | V2 view, scale) -> the modules to unbind."""
        if torch.is_grad_enabled():
            raise RuntimeError('an image-prompt state under enabled autograd: IP-Adapter conditioning is forward only (use torch.no_grad())')
        if ops._dual is not None:
            raise RuntimeError('an image-prompt state inside a grouped pass (forward_pair / ops.dual_networks): the adapter has no partner network')
        if 'fp8' in unet._flat:
            raise RuntimeError('an image-prompt state with an e4m3-weight UNet (enable_fp8_weights): not supported')
        ad = self.adapter
        if ad.compute_dtype != unet.compute_dtype:
            raise RuntimeError(f'the IP-Adapter computes in {ad.compute_dtype}, the UNet in {unet.compute_dtype}')
        if ad.cross_attention_dim != unet.cfg.cross_attention_dim:
            raise ValueError(f'IP-Adapter and UNet differ in cross_attention_dim: {ad.cross_attention_dim} vs {unet.cfg.cross_attention_dim}')
        layers = unet.cross_attention_layers()
        if len(layers) != len(ad.channels):
            raise ValueError(f'the IP-Adapter has {len(ad.channels)} layers, the UNet {len(layers)} cross-attention layers')
        for i, (m, c) in enumerate(zip(layers, ad.channels)):
            if m.to_q.weight.shape[0] != c:
                raise ValueError(f'IP-Adapter layer {2 * i + 1} has {c} channels, the UNet\'s cross-attention layer {i} has {m.to_q.weight.shape[0]}')
        if self.kv.shape[0] != x.shape[0]:
            raise ValueError(f'image-prompt state for {self.kv.shape[0]} rows, UNet input {x.shape[0]} rows: one image per sample and `dup` '
                             'must match the guidance batch')
        for i, m in enumerate(layers):
            m.ip = (self.layer_kv(i), self.scale)
        return layers


class HipIPAdapter:
    """`prepare(image_embeds, scale, dup)` / `prepare_images(images_u8, tower, scale, dup)` -> IPState.  fp32 masters under the published
    key names (`state_dict()`); compute copies in the UNet's compute dtype, the layers' to_k_ip | to_v_ip concatenated row-wise."""

    def __init__(self, cfg, state, device, compute_dtype=BF16, embed_dim=None, where='IP-Adapter state'):
        if compute_dtype not in (BF16, F32):
            raise ValueError('compute_dtype must be torch.bfloat16 or torch.float32')
        state = flatten_state(state, where)
        self.tokens = check_state_dict(state, cfg, embed_dim, where)
        self.cfg, self.compute_dtype, self.device = cfg, compute_dtype, torch.device(device)
        self.cross_attention_dim = cfg.cross_attention_dim
        self.embed_dim = state['image_proj.proj.weight'].shape[1]
        if self.embed_dim % 8:
            raise ValueError(f'{where}: embedding width E = {self.embed_dim}: the GEMM kernels take multiples of 8')
        self.masters = {k: state[k].detach().to(self.device, F32).contiguous() for k in expected_keys(cfg)}
        table = layer_table(cfg)
        self.channels = [c for _, _, c in table]
        self.offsets, off = [], 0
        for c in self.channels:
            self.offsets.append(off)
            off += 2 * c
        self.width = off
        m, cd = self.masters, compute_dtype
        self.w_proj = m['image_proj.proj.weight'].to(cd)
        self.b_proj = m['image_proj.proj.bias']
        self.ln = (m['image_proj.norm.weight'], m['image_proj.norm.bias'])
        self.w_kv = torch.cat([m[f'ip_adapter.{n}.to_{p}_ip.weight'] for n, _, _ in table for p in 'kv']).to(cd).contiguous()   # [sum 2 C_l, Dctx]

    def state_dict(self):
        return {k: v.detach().cpu() for k, v in self.masters.items()}

    @torch.no_grad()
    def project(self, image_embeds):
        """[B, E] fp32 -> the image tokens [B * T, Dctx] (compute dtype): one GEMM with bias, one LayerNorm."""
        if not torch.is_tensor(image_embeds) or image_embeds.dim() != 2 or image_embeds.shape[1] != self.embed_dim:
            got = tuple(image_embeds.shape) if torch.is_tensor(image_embeds) else type(image_embeds).__name__
            raise ValueError(f'image embeddings {got}: expected [B, {self.embed_dim}]')
        if image_embeds.device.type != 'cuda':
            raise RuntimeError('HipIPAdapter runs on the GPU only (no CPU fallback)')
        a = image_embeds.to(self.compute_dtype).contiguous()
        t = ops.gemm(a, self.w_proj, bias=self.b_proj)                                     # [B, T * Dctx]
        return ops.layer_norm(t.view(-1, self.cross_attention_dim), *self.ln, LN_EPS)      # [B * T, Dctx]

    @torch.no_grad()
    def prepare(self, image_embeds, scale=1.0, dup=1):
        """image_embeds [B, E] fp32 (HipCLIPVisionTower's output) -> IPState for UNet inputs of dup * B rows.  dup = 2: the [uncond ; cond]
        halves of a guided batch; the uncond half takes the projection of zero embeddings.  Three GEMM / LayerNorm launches, once."""
        scale = float(scale)
        if not scale >= 0 or scale == float('inf'):
            raise ValueError(f'image-prompt scale {scale}: expected a finite value >= 0')
        if dup not in (1, 2):
            raise ValueError(f'dup {dup}: expected 1 or 2')
        e = image_embeds.to(F32) if torch.is_tensor(image_embeds) else image_embeds
        if dup == 2 and torch.is_tensor(e) and e.dim() == 2:
            e = torch.cat([torch.zeros_like(e), e])
        tokens = self.project(e)
        kv = ops.gemm(tokens, self.w_kv)                                                    # [dup * B * T, sum 2 C_l]
        n = tokens.shape[0] // self.tokens
        return IPState(self, tokens.view(n, self.tokens, -1), kv.view(n, self.tokens, self.width), scale)

    @torch.no_grad()
    def prepare_images(self, images_u8, tower, scale=1.0, dup=1):
        """uint8 [B, 3, H, W] prompt images -> IPState through `tower`, a clip.HipCLIPVisionTower(preprocess='pil')."""
        if getattr(tower, 'preprocess', None) != 'pil':
            raise ValueError("prepare_images: the image encoder must be a HipCLIPVisionTower(preprocess='pil') (the CLIPImageProcessor transform)")
        if tower.cfg.projection_dim != self.embed_dim:
            raise ValueError(f'the IP-Adapter takes embeddings of width E = {self.embed_dim}, the image encoder has projection_dim '
                             f'{tower.cfg.projection_dim}')
        return self.prepare(tower(images_u8).to(F32), scale, dup)


def load_ip_adapter(spec, unet, device, embed_dim, seed=0):
    """An IP-Adapter for `unet` (its configuration and compute dtype) and an image encoder of projection_dim `embed_dim`: a local
    `.safetensors` / `.bin` file, or 'random:ip-adapter[:seed]' (seeded NON-zero weights, T = 4)."""
    name = str(spec)
    if name.lower().startswith('random:'):
        s = parse_random_spec(name)
        sd = random_state_dict(unet.cfg, embed_dim, seed if s is None else s)
    else:
        sd = read_state_file(name)
    return HipIPAdapter(unet.cfg, sd, device, unet.compute_dtype, embed_dim, where=name)
