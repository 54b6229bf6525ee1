"""ControlNet (Zhang et al. 2023) on the HIP kernels, forward only: diffusers' `ControlNetModel` for the SD1.5 / SD2.1-base UNets.

A ControlNet is a copy of the UNet's encoder (`conv_in`, `time_embedding`, `down_blocks`, `mid_block`: the block classes of unet.py, built
by HipUNet2DCondition._build_encoder) plus a hint embedder of eight 3 x 3 convolutions, thirteen 1 x 1 "zero convolutions" and one addition
per skip connection.  Parameter names and shapes are diffusers', so a `diffusion_pytorch_model.safetensors` loads with `load_state_dict`.

Everything runs on the UNet's kernels, NHWC, in the UNet's compute dtype (bf16 or fp32):
  * the control images become the embedder's input in ONE launch (ops.control_hint_u8, csrc/controlnet.hip), the embedder's SiLUs are
    the convolutions' epilogue flag, and `conv_in(x) + e` is conv_in's residual epilogue;
  * the embedding `e` is computed once per batch (HipControlNet.prepare -> ControlState), never inside a sampling loop;
  * a tap, `skip + s (W f + b)`, is one GEMM with the UNet's tensor as its res operand; the scale s is folded into the tap's compute
    weights and bias when the state is prepared (HipUNet2DCondition.forward_nhwc(control=...)).
The parameters live in flat buffers as the UNet's do (HipUNet2DCondition.materialize) without gradient buffers and without
backward-data operands.

These rules restate diffusers' `ControlNetModel` and the residual rule of `UNet2DConditionModel`; the package is not installed here, so
agreement with it is not pinned by a test (tests/controlnet_ref.py is a torch.nn restatement of the same rules).
"""
import json
import os

import torch
import torch.nn as nn

from . import ops
from .unet import BF16, CONFIGS, F32, HConv1x1, HConv3x3, HipUNet2DCondition, UNetConfig, _TembSlices, unet_forward_macs

SD_COND_CHANNELS = (16, 32, 96, 256)       # diffusers' conditioning_embedding_out_channels
TINY_COND_CHANNELS = (8, 16, 24, 32)       # for the tiny configurations of unet.CONFIGS
RANDOM_PREFIX = 'random:controlnet'


def default_cond_channels(cfg):
    return SD_COND_CHANNELS if cfg.block_out_channels[0] >= 320 else TINY_COND_CHANNELS


def tap_channels(cfg):
    """Channel counts of the twelve skip features (conv_in's output first), in the order `controlnet_down_blocks` taps them."""
    ch = cfg.block_out_channels
    out = [ch[0]]
    for i, c in enumerate(ch):
        out += [c] * (cfg.layers_per_block + (i != len(ch) - 1))
    return out


class ControlNetConditioningEmbedding(nn.Module):
    """diffusers' hint embedder: conv_in, six `blocks` (every second one stride 2: 8h x 8w pixels -> h x w), conv_out; SiLU after all but
    conv_out.  The image's 3 channels arrive as 8 (channels 3..7 zero), conv_in's compute copy is zero-padded to match."""

    def __init__(self, out_channels, cond_channels):
        super().__init__()
        c = tuple(cond_channels)
        self.conv_in = HConv3x3(3, c[0])
        self.blocks = nn.ModuleList()
        for i in range(len(c) - 1):
            self.blocks.append(HConv3x3(c[i], c[i]))
            self.blocks.append(HConv3x3(c[i], c[i + 1], stride=2))
        self.conv_out = HConv3x3(c[-1], out_channels)

    def forward(self, hint):
        e = ops.conv3x3(hint, self.conv_in.w16, bias=self.conv_in.bias, silu=True)
        for blk in self.blocks:
            e = ops.conv3x3(e, blk.w16, bias=blk.bias, stride=blk.stride, silu=True)
        return ops.conv3x3(e, self.conv_out.w16, bias=self.conv_out.bias)


def check_controlnet_config(config, cfg, where='ControlNet config'):
    """A diffusers ControlNetModel config (the dict of its config.json) against the UNet configuration `cfg` -> its
    conditioning_embedding_out_channels.  Anything this module does not reproduce, or that differs from the UNet, is a ValueError that
    names the key."""
    for key in ('global_pool_conditions', 'class_embed_type', 'addition_embed_type'):
        if config.get(key):
            raise ValueError(f'{where}: {key} = {config[key]!r} is not supported')
    if config.get('conditioning_channels', 3) != 3:
        raise ValueError(f"{where}: conditioning_channels = {config['conditioning_channels']!r}: the control image is 3-channel RGB")
    n = len(cfg.block_out_channels)
    heads = config.get('num_attention_heads') or config.get('attention_head_dim', 8)
    heads = tuple(heads) if isinstance(heads, (list, tuple)) else (heads,) * n
    for key, got, want in (('block_out_channels', tuple(config.get('block_out_channels', (320, 640, 1280, 1280))), tuple(cfg.block_out_channels)),
                           ('cross_attention_dim', config.get('cross_attention_dim', 1280), cfg.cross_attention_dim),
                           ('use_linear_projection', bool(config.get('use_linear_projection', False)), cfg.use_linear_projection),
                           ('attention_head_dim', heads, tuple(cfg.num_heads)),
                           ('layers_per_block', config.get('layers_per_block', 2), cfg.layers_per_block),
                           ('norm_num_groups', config.get('norm_num_groups', 32), cfg.norm_num_groups)):
        if got != want:
            raise ValueError(f'{where}: {key} = {got!r}, the UNet has {want!r}: a ControlNet is a copy of its UNet\'s encoder')
    cond = tuple(config.get('conditioning_embedding_out_channels', SD_COND_CHANNELS))
    if len(cond) != 4 or any(c <= 0 or c % 8 for c in cond):
        raise ValueError(f'{where}: conditioning_embedding_out_channels = {cond!r}: expected four positive multiples of 8')
    return cond


def check_same_architecture(control_cfg, unet_cfg):
    """The fields of unet.UNetConfig that fix the shapes of the skip features and of the text states: a mismatch names the field."""
    for key in ('block_out_channels', 'cross_attention_dim', 'use_linear_projection', 'num_heads', 'layers_per_block', 'down_has_attn',
                'norm_num_groups', 'in_channels'):
        a, b = getattr(control_cfg, key), getattr(unet_cfg, key)
        if a != b:
            raise ValueError(f'ControlNet and UNet differ in {key}: {a!r} vs {b!r}')


def parse_random_spec(spec):
    """'random:controlnet' -> None (the caller's seed), 'random:controlnet:<seed>' -> the seed; any other 'random:...' is a ValueError."""
    parts = str(spec).lower().split(':')
    if parts[:2] != RANDOM_PREFIX.split(':') or len(parts) > 3:
        raise ValueError(f"{spec}: expected '{RANDOM_PREFIX}' or '{RANDOM_PREFIX}:<seed>'")
    if len(parts) == 2:
        return None
    if not parts[2].isdigit():
        raise ValueError(f'{spec}: the seed must be a non-negative integer')
    return int(parts[2])


class ControlState:
    """What a sampling loop carries: the hint embedding `e` [dup * B, h, w, C0] (computed once), the scale and the thirteen taps with the
    scale folded into their compute weights and biases.  Made by HipControlNet.prepare; consumed by forward_nhwc(control=...)."""

    def __init__(self, net, e, scale, taps):
        self.net, self.e, self.scale, self.taps = net, e, float(scale), taps

    def features(self, unet, x, timesteps, ctx):
        """The checks of a controlled pass, then the ControlNet's twelve skip features and its mid feature on the UNet's inputs."""
        if torch.is_grad_enabled():
            raise RuntimeError('a control state under enabled autograd: ControlNet conditioning is forward only (use torch.no_grad())')
        if ops._dual is not None:
            raise RuntimeError('a control state inside a grouped pass (forward_pair / ops.dual_networks): the ControlNet has no partner network')
        if 'fp8' in unet._flat:
            raise RuntimeError('a control state with an e4m3-weight UNet (enable_fp8_weights): not supported')
        net = self.net
        check_same_architecture(net.cfg, unet.cfg)
        if net.compute_dtype != unet.compute_dtype:
            raise RuntimeError(f'the ControlNet computes in {net.compute_dtype}, the UNet in {unet.compute_dtype}')
        if tuple(self.e.shape[:3]) != tuple(x.shape[:3]):
            b, h, w = self.e.shape[:3]
            raise ValueError(f'control state for {b} rows of {h} x {w} latents (control images {8 * h} x {8 * w}), UNet input '
                             f'{x.shape[0]} rows of {x.shape[1]} x {x.shape[2]}: the control image must be exactly 8h x 8w and `dup` must '
                             'match the guidance batch')
        return net.features(x, timesteps, ctx, self.e)

    def inject(self, i, feat, target):
        """target + s (W_i feat + b_i): one GEMM, the UNet's tensor is the residual operand."""
        weight, w16, bias = self.taps[i]
        B, H, W, C = target.shape
        return ops.linear(feat.view(B * H * W, C), weight, bias, w16, None, res=target.view(B * H * W, C)).view(B, H, W, C)


class HipControlNet(HipUNet2DCondition):
    """`prepare(images_u8, scale, dup)` -> ControlState; `features(x, t, ctx, e)` -> the thirteen features the taps read.  Shares the flat
    parameter storage, the fused time-embedding projection and the fused q|k|v projections with HipUNet2DCondition (materialize,
    refresh_compute_weights, load_state_dict, state_dict); it has no up blocks, no gradient buffers and no backward-data operands, and
    the training-side members of the base class (grouped passes, e4m3 copies, cloning, pickling) are refused."""

    backward_operands = False

    def __init__(self, cfg: UNetConfig = None, cond_channels=None, device=None, seed=None, compute_dtype=BF16):
        nn.Module.__init__(self)
        cfg = cfg or CONFIGS['sd15']
        if compute_dtype not in (BF16, F32):
            raise ValueError('compute_dtype must be torch.bfloat16 or torch.float32')
        self.cfg, self.compute_dtype = cfg, compute_dtype
        self.cond_channels = tuple(cond_channels or default_cond_channels(cfg))
        if any(c <= 0 or c % 8 for c in self.cond_channels) or len(self.cond_channels) != 4:
            raise ValueError(f'cond_channels {self.cond_channels!r}: expected four positive multiples of 8')
        ch = cfg.block_out_channels
        with torch.device('meta'):
            self._build_encoder()
            self.controlnet_cond_embedding = ControlNetConditioningEmbedding(ch[0], self.cond_channels)
            self.controlnet_down_blocks = nn.ModuleList([HConv1x1(c, c) for c in tap_channels(cfg)])
            self.controlnet_mid_block = HConv1x1(ch[-1], ch[-1])
        self._flat = None
        self._grad_ready_cb = None
        self._train_params = False
        if device is not None:
            self.materialize(device, seed=seed)

    def materialize(self, device, seed=None, with_grad_buffers=False, source=None):
        """As HipUNet2DCondition.materialize, always without gradient buffers.  Seeded init (`source` None): fan-in-scaled NON-zero
        values for every convolution, the taps and the embedder's conv_out included (see sd_util.load_controlnet)."""
        if with_grad_buffers:
            raise ValueError('HipControlNet is forward only: it has no gradient buffers')
        super().materialize(device, seed=seed, with_grad_buffers=False, source=source)
        return self.requires_grad_(False)

    def _taps(self):
        return list(self.controlnet_down_blocks) + [self.controlnet_mid_block]

    @torch.no_grad()
    def prepare(self, images_u8, scale=1.0, dup=1):
        """images_u8: uint8 [B, 8h, 8w, 3] RGB on the GPU -> ControlState for UNet inputs of dup * B rows of h x w latents (dup = 2: the
        [uncond ; cond] halves of a guided batch get the same hint, as in diffusers' pipeline).  One conversion launch and the eight
        convolutions of the embedder, once; the scale is folded into the taps here: compute weights (W * s in fp32, then cast), bias b * s."""
        if self._flat is None:
            raise RuntimeError('HipControlNet is not materialised on a GPU')
        if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
            got = f'{images_u8.dtype} {tuple(images_u8.shape)}' if torch.is_tensor(images_u8) else type(images_u8).__name__
            raise ValueError(f'control images: expected uint8 [B, H, W, 3], got {got}')
        H, W = images_u8.shape[1:3]
        if H % 8 or W % 8 or not H or not W:
            raise ValueError(f'control images {H} x {W}: both sides must be positive multiples of 8 (8h x 8w for h x w latents)')
        scale = float(scale)
        if not scale >= 0:
            raise ValueError(f'control scale {scale}: expected a value >= 0')
        if dup not in (1, 2):
            raise ValueError(f'dup {dup}: expected 1 or 2')
        self._sync_foreign_state()
        cd = self.compute_dtype
        e = self.controlnet_cond_embedding(ops.control_hint_u8(images_u8.contiguous(), cd))
        if dup > 1:
            e = e.repeat(dup, 1, 1, 1)
        taps = []
        for m in self._taps():
            if scale == 1:
                taps.append((m.weight, m.w16, m.bias))
            else:
                w = (m.weight.reshape(m.weight.shape[0], -1) * scale).to(cd).contiguous()
                taps.append((m.weight, w, (m.bias * scale).contiguous()))
        return ControlState(self, e, scale, taps)

    def features(self, x, timesteps, ctx, e):
        """x, timesteps, ctx as forward_nhwc takes them, e: the hint embedding [N, h, w, C0] -> the twelve skip features + the mid feature."""
        cfg = self.cfg
        temb = self.time_embedding(ops.timestep_embed(timesteps, cfg.block_out_channels[0], self.compute_dtype))
        f = self.fused
        tall = ops.linear(ops.silu(temb), f['w'], f['b'], f['w16'], f['w16t'], out_f32=True)
        temb_act = _TembSlices(tall, self._temb_cols)
        ctx2d = ctx.reshape(-1, ctx.shape[-1])
        h = self.conv_in(x, res=e)                       # conv_in(x) + e: the residual epilogue
        feats = [h]
        for blk in self.down_blocks:
            h, outs = blk(h, temb_act, ctx2d)
            feats.extend(outs)
        feats.append(self.mid_block(h, temb_act, ctx2d))
        return feats

    # ---- members of the base class that do not apply to a forward-only network
    def _refuse(self, what):
        raise RuntimeError(f'HipControlNet: {what} is not supported (forward only, bf16 or fp32 weights)')

    def enable_fp8_weights(self, *a, **k):
        self._refuse('enable_fp8_weights')

    def forward_pair(self, *a, **k):
        self._refuse('a grouped pass')

    def partner_map(self, other):
        self._refuse('a grouped pass')

    def clone_network(self, *a, **k):
        self._refuse('clone_network')

    def __getstate__(self):
        self._refuse('pickling (load it from its directory or spec)')

    def forward_nhwc(self, *a, **k):
        self._refuse('forward_nhwc (use prepare() and HipUNet2DCondition.forward_nhwc(control=...))')

    forward = forward_nhwc


def controlnet_forward_macs(cfg, h, w, cond_channels=None):
    """-> (per step, prepare): multiply-accumulates of one ControlNet pass on one sample of h x w latents (the encoder copy and the thirteen
    1 x 1 taps: what a controlled UNet pass adds to unet_forward_macs) and of the one-off hint embedder on its 8h x 8w image (the padded
    input channels of its conv_in not counted)."""
    enc, taps = unet_forward_macs(cfg, h, w, encoder_only=True)
    step = enc + sum(c * c * n for c, n in taps)
    c = tuple(cond_channels or default_cond_channels(cfg))
    n = 64 * h * w
    prep = n * 9 * 3 * c[0]
    for i in range(len(c) - 1):
        prep += n * 9 * c[i] * c[i]
        n //= 4
        prep += n * 9 * c[i] * c[i + 1]
    return step, prep + n * 9 * c[-1] * cfg.block_out_channels[0]


def load_controlnet_dir(path, unet, device):
    """A local directory in diffusers' layout (config.json, diffusion_pytorch_model.safetensors) -> HipControlNet of the UNet's
    architecture and compute dtype.  The config is checked against the UNet (check_controlnet_config); a missing key or a wrong shape
    in the weights file is a ValueError that names it."""
    cj, wf = os.path.join(path, 'config.json'), os.path.join(path, 'diffusion_pytorch_model.safetensors')
    for f in (cj, wf):
        if not os.path.isfile(f):
            raise FileNotFoundError(f'{f}: not found (a ControlNet directory holds config.json and diffusion_pytorch_model.safetensors)')
    with open(cj) as f:
        cond = check_controlnet_config(json.load(f), unet.cfg, where=cj)
    from safetensors.torch import load_file
    src = load_file(wf)
    net = HipControlNet(unet.cfg, cond_channels=cond, compute_dtype=unet.compute_dtype)
    check_state_dict(src, net, wf)
    return net.materialize(device, source=src)


def check_state_dict(src, net, where):
    """Every parameter of `net` must be in `src` with its shape; the first one that is not is named."""
    for name, p in net.named_parameters():
        if name not in src:
            raise ValueError(f'{where}: missing key {name}')
        if tuple(src[name].shape) != tuple(p.shape):
            raise ValueError(f'{where}: {name} has shape {tuple(src[name].shape)}, expected {tuple(p.shape)}')
    extra = sorted(set(src) - {n for n, _ in net.named_parameters()})
    if extra:
        raise ValueError(f'{where}: unexpected key {extra[0]}' + (f' (and {len(extra) - 1} more)' if len(extra) > 1 else ''))
