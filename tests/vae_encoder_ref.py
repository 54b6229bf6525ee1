"""fp32 PyTorch restatement of the AutoencoderKL *encoder* of Stable Diffusion (diffusers `Encoder` + `quant_conv` +
`DiagonalGaussianDistribution`), the yardstick of tests/test_gpu_vae_encoder.py.  A helper, not a test.

Nothing in the reference project encodes images, so there is no reference program to pin to; this follows the published diffusers
architecture for SD 1.x / 2.x:
  conv_in 3x3 (3 -> 128) -> 4 down blocks with (128, 256, 512, 512) channels, `layers_per_block` ResBlocks each, and after the first
  three a Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)) then conv3x3 stride 2 without padding -> mid: ResBlock, single-head
  attention, ResBlock -> GroupNorm(32, eps 1e-6) -> SiLU -> conv_out 3x3 (512 -> 8) -> quant_conv 1x1 (8 -> 8) -> mean | logvar,
  logvar clamped to [-30, 20], std = exp(logvar / 2).
The blocks shared with the decoder (ResBlock, attention, mid block) and the configurations are those of oracle/vae_ref.py (import
only).  Parameter names equal diffusers' `state_dict` keys, i.e. those of sid_lsg_amd.vae.HipAutoencoderKLEncoder.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.vae_ref import VAE_CONFIGS, ResnetRef, VAEConfig, _Mid  # noqa: F401


def downsample_br(x, weight, bias):
    """diffusers Downsample2D(padding=0), literally: pad right and bottom by one, stride-2 conv without padding."""
    return F.conv2d(F.pad(x, (0, 1, 0, 1), mode='constant', value=0.0), weight, bias, stride=2, padding=0)


class _Down(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, stride=2, padding=0)

    def forward(self, x):
        return downsample_br(x, self.conv.weight, self.conv.bias)


class _DownBlock(nn.Module):
    def __init__(self, cin, cout, n, groups, add_down):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetRef(cin if i == 0 else cout, cout, groups) for i in range(n)])
        self.downsamplers = nn.ModuleList([_Down(cout)]) if add_down else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return x if self.downsamplers is None else self.downsamplers[0](x)


class EncoderRef(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        ch = list(cfg.block_out_channels)
        g = cfg.norm_num_groups
        self.conv_in = nn.Conv2d(cfg.out_channels, ch[0], 3, padding=1)
        self.down_blocks = nn.ModuleList()
        prev = ch[0]
        for i, c in enumerate(ch):
            self.down_blocks.append(_DownBlock(prev, c, cfg.layers_per_block, g, add_down=i < len(ch) - 1))
            prev = c
        self.mid_block = _Mid(ch[-1], g)
        self.conv_norm_out = nn.GroupNorm(g, ch[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(ch[-1], 2 * cfg.latent_channels, 3, padding=1)

    def forward(self, x):
        h = self.conv_in(x)
        for b in self.down_blocks:
            h = b(h)
        return self.conv_out(F.silu(self.conv_norm_out(self.mid_block(h))))


class GaussianRef:
    def __init__(self, moments):
        self.mean, logvar = moments.chunk(2, dim=1)
        self.logvar = logvar.clamp(-30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)

    def mode(self):
        return self.mean

    def sample(self, eps):
        return self.mean + self.std * eps


class AutoencoderKLEncoderRef(nn.Module):
    """`.encode(x).latent_dist` for x fp32 [B, 3, H, W] in [-1, 1]."""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.encoder = EncoderRef(cfg)
        self.quant_conv = nn.Conv2d(2 * cfg.latent_channels, 2 * cfg.latent_channels, 1)

    @torch.no_grad()
    def encode(self, x):
        return GaussianRef(self.quant_conv(self.encoder(x)))
