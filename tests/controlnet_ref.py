"""Reference for the ControlNet tests: a plain torch.nn restatement (NCHW, any float dtype; the tests run it in fp64) of diffusers'
`ControlNetModel` and of the residual rule of `UNet2DConditionModel`, built from the block classes of oracle/unet_ref.py.  Parameter
names and shapes are diffusers', so the HIP modules and this reference load ONE state dict.  TEST INFRASTRUCTURE ONLY."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.unet_ref import CONFIGS, DownBlock, MidBlock, TimestepEmbedding, UNet2DConditionRef, UNetOutput, timestep_embedding

SD_COND_CHANNELS = (16, 32, 96, 256)
TINY_COND_CHANNELS = (8, 16, 24, 32)


def cond_channels_of(cfg):
    return SD_COND_CHANNELS if cfg.block_out_channels[0] >= 320 else TINY_COND_CHANNELS


class ConditioningEmbeddingRef(nn.Module):
    def __init__(self, out_channels, c):
        super().__init__()
        self.conv_in = nn.Conv2d(3, c[0], 3, padding=1)
        self.blocks = nn.ModuleList()
        for i in range(len(c) - 1):
            self.blocks.append(nn.Conv2d(c[i], c[i], 3, padding=1))
            self.blocks.append(nn.Conv2d(c[i], c[i + 1], 3, padding=1, stride=2))
        self.conv_out = nn.Conv2d(c[-1], out_channels, 3, padding=1)

    def forward(self, cond):
        e = F.silu(self.conv_in(cond))
        for blk in self.blocks:
            e = F.silu(blk(e))
        return self.conv_out(e)


class ControlNetRef(nn.Module):
    """forward(sample, t, ctx, cond [B, 3, 8h, 8w] in [0, 1], scale) -> (twelve down residuals, mid residual), each already times scale."""

    def __init__(self, cfg, cond_channels=None):
        super().__init__()
        self.cfg = cfg
        ch = cfg.block_out_channels
        self.conv_in = nn.Conv2d(cfg.in_channels, ch[0], 3, padding=1)
        self.time_embedding = TimestepEmbedding(ch[0], cfg.time_embed_dim)
        self.down_blocks = nn.ModuleList()
        taps = [ch[0]]
        cout = ch[0]
        for i, c in enumerate(ch):
            cin, cout = cout, c
            last = i == len(ch) - 1
            self.down_blocks.append(DownBlock(cfg, cin, cout, cfg.num_heads[i], cfg.down_has_attn[i], add_down=not last))
            taps += [c] * (cfg.layers_per_block + (not last))
        self.mid_block = MidBlock(cfg, ch[-1], cfg.num_heads[-1])
        self.controlnet_cond_embedding = ConditioningEmbeddingRef(ch[0], tuple(cond_channels or cond_channels_of(cfg)))
        self.controlnet_down_blocks = nn.ModuleList([nn.Conv2d(c, c, 1) for c in taps])
        self.controlnet_mid_block = nn.Conv2d(ch[-1], ch[-1], 1)

    def embed(self, cond):
        return self.controlnet_cond_embedding(cond)

    def features(self, sample, t, ctx, cond):
        temb = self.time_embedding(timestep_embedding(t, self.cfg.block_out_channels[0]).to(sample.dtype))
        x = self.conv_in(sample) + self.embed(cond)
        feats = [x]
        for blk in self.down_blocks:
            x, outs = blk(x, temb, ctx)
            feats.extend(outs)
        feats.append(self.mid_block(x, temb, ctx))
        return feats

    def forward(self, sample, t, ctx, cond, scale=1.0):
        feats = self.features(sample, t, ctx, cond)
        down = [tap(f) * scale for tap, f in zip(self.controlnet_down_blocks, feats[:-1])]
        return down, self.controlnet_mid_block(feats[-1]) * scale


class ControlledUNetRef(UNet2DConditionRef):
    """UNet2DConditionRef whose forward takes the thirteen residuals: every skip gets its residual after the down blocks (the mid block's
    input stays the last down block's own output), the mid block's output gets the mid residual."""

    def forward(self, sample, timestep, encoder_hidden_states=None, down_residuals=None, mid_residual=None, **_):
        if down_residuals is None and mid_residual is None:
            return super().forward(sample, timestep, encoder_hidden_states)
        cfg = self.cfg
        t = timestep.expand(sample.shape[0])
        temb = self.time_embedding(timestep_embedding(t, cfg.block_out_channels[0]).to(sample.dtype))
        x = self.conv_in(sample)
        skips = [x]
        for blk in self.down_blocks:
            x, outs = blk(x, temb, encoder_hidden_states)
            skips.extend(outs)
        assert len(skips) == len(down_residuals)
        skips = [s + r for s, r in zip(skips, down_residuals)]
        x = self.mid_block(x, temb, encoder_hidden_states) + mid_residual
        for blk in self.up_blocks:
            x = blk(x, skips, temb, encoder_hidden_states)
        return UNetOutput(self.conv_out(F.silu(self.conv_norm_out(x))))


def make_pair(cfg_name, unet_seed=1234, control_seed=0, dtype=torch.float64):
    """(ControlledUNetRef, ControlNetRef, unet state dict, controlnet state dict): the seeded weights of HipUNet2DCondition /
    HipControlNet (unet.random_parameters: one CPU stream per network), loaded through their diffusers key names."""
    from sid_lsg_amd.controlnet import HipControlNet
    from sid_lsg_amd.unet import CONFIGS as HC, random_state_dict, random_parameters, _random_parameter_slots
    cfg = CONFIGS[cfg_name]
    usd = random_state_dict(HC[cfg_name], unet_seed)
    net = HipControlNet(HC[cfg_name])
    names = {id(m): n for n, m in net.named_modules()}
    csd = {f'{names[id(mod)]}.{pname}': v for (mod, pname), v in zip(_random_parameter_slots(net), random_parameters(net, control_seed))}
    unet = ControlledUNetRef(cfg)
    unet.load_state_dict(usd)
    cnet = ControlNetRef(cfg)
    cnet.load_state_dict(csd)
    return unet.to(dtype).eval().requires_grad_(False), cnet.to(dtype).eval().requires_grad_(False), usd, csd


def make_inputs(cfg_name, B=3, h=8, w=12, seed=0):
    """x [B, 4, h, w], distinct timesteps [B], ctx [B, L, D] (bf16-representable), control images uint8 [B, 8h, 8w, 3]."""
    cfg = CONFIGS[cfg_name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, h, w, generator=g).to(torch.bfloat16).float()
    t = torch.tensor([625, 37, 981, 250, 4][:B])
    ctx = torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g).to(torch.bfloat16).float()
    img = torch.randint(0, 256, (B, 8 * h, 8 * w, 3), generator=g, dtype=torch.uint8)
    return x, t, ctx, img


def ref_outputs(unet, cnet, x, t, ctx, img, scale=1.0):
    """fp64: (plain UNet output, controlled UNet output) [B, 4, h, w]."""
    d = next(unet.parameters()).dtype
    x, ctx = x.to(d), ctx.to(d)
    cond = (img.to(d) / 255).permute(0, 3, 1, 2)
    with torch.no_grad():
        plain = unet(x, t, encoder_hidden_states=ctx).sample
        down, mid = cnet(x, t, ctx, cond, scale)
        ctl = unet(x, t, encoder_hidden_states=ctx, down_residuals=down, mid_residual=mid).sample
    return plain, ctl
