"""Reference for the IP-Adapter tests: a plain torch.nn restatement (NCHW, any float dtype; the tests run it in fp64) of the published
IP-Adapter modules for SD 1.5 -- the linear image projection and the decoupled cross-attention processor -- on oracle/unet_ref.py's
UNet2DConditionRef, each `attn2` wrapped to add s * attn(q, to_k_ip(tokens), to_v_ip(tokens)).  It loads the state dict the HIP module
loads, through the published key names.  TEST INFRASTRUCTURE ONLY."""
import torch
import torch.nn as nn

from controlnet_ref import ControlledUNetRef
from oracle.unet_ref import CONFIGS

TOKENS = 4
EMBED_DIM = 32        # projection_dim of clip.CLIP_ARCHS['tiny']


class ImageProjRef(nn.Module):
    """image_embeds [B, E] -> tokens [B, T, Dctx]: LayerNorm(reshape(Linear(e)))."""

    def __init__(self, embed_dim, dctx, tokens):
        super().__init__()
        self.tokens, self.dctx = tokens, dctx
        self.proj = nn.Linear(embed_dim, tokens * dctx)
        self.norm = nn.LayerNorm(dctx, eps=1e-5)

    def forward(self, e):
        return self.norm(self.proj(e).reshape(-1, self.tokens, self.dctx))


class IPAttnRef(nn.Module):
    """An oracle Attention (a UNet's attn2) with the decoupled image attention added in front of to_out."""

    def __init__(self, attn, dctx):
        super().__init__()
        self.attn = attn
        c = attn.to_q.in_features
        self.to_k_ip = nn.Linear(dctx, c, bias=False)
        self.to_v_ip = nn.Linear(dctx, c, bias=False)
        self.tokens, self.scale = None, 1.0

    def forward(self, x, ctx=None):
        a = self.attn
        B, N, C = x.shape
        h, d = a.heads, C // a.heads
        split = lambda t: t.view(B, -1, h, d).transpose(1, 2)      # noqa: E731
        q = split(a.to_q(x))

        def att(k, v):
            p = torch.softmax(torch.matmul(q, split(k).transpose(-1, -2)) * (d ** -0.5), dim=-1)
            return torch.matmul(p, split(v)).transpose(1, 2).reshape(B, N, C)

        o = att(a.to_k(ctx), a.to_v(ctx))
        if self.tokens is not None:
            o = o + self.scale * att(self.to_k_ip(self.tokens), self.to_v_ip(self.tokens))
        return a.to_out[0](o)


class IPAdapterRef(nn.Module):
    """The adapter attached to a UNet2DConditionRef: wraps its attn2 modules in the order down blocks, up blocks, mid block and names
    them ip_adapter.<2 i + 1>."""

    def __init__(self, unet, embed_dim=EMBED_DIM, tokens=TOKENS):
        super().__init__()
        dctx = unet.cfg.cross_attention_dim
        self.image_proj = ImageProjRef(embed_dim, dctx, tokens)
        self.layers = []
        for blk in list(unet.down_blocks) + list(unet.up_blocks) + [unet.mid_block]:
            for tr in getattr(blk, 'attentions', None) or ():
                for b in tr.transformer_blocks:
                    b.attn2 = IPAttnRef(b.attn2, dctx)
                    self.layers.append(b.attn2)

    def load_published(self, sd):
        d = next(self.image_proj.parameters()).dtype
        self.image_proj.load_state_dict({k[len('image_proj.'):]: v.to(d) for k, v in sd.items() if k.startswith('image_proj.')})
        for i, m in enumerate(self.layers):
            m.to_k_ip.weight.data.copy_(sd[f'ip_adapter.{2 * i + 1}.to_k_ip.weight'])
            m.to_v_ip.weight.data.copy_(sd[f'ip_adapter.{2 * i + 1}.to_v_ip.weight'])
        assert len(sd) == 4 + 2 * len(self.layers)
        return self

    def set(self, tokens, scale=1.0):
        """tokens [B, T, Dctx] (image_proj's output), or None: the plain UNet."""
        for m in self.layers:
            m.tokens, m.scale = tokens, float(scale)

    def layer_kv(self, tokens):
        return [(m.to_k_ip(tokens), m.to_v_ip(tokens)) for m in self.layers]


def make_ref(cfg_name, unet_seed=1234, adapter_seed=0, dtype=torch.float64, usd=None):
    """(ControlledUNetRef with wrapped attn2, IPAdapterRef, unet state dict, adapter state dict): seeded weights (or the UNet state dict
    `usd`), loaded through the key names the HIP modules load them by."""
    from sid_lsg_amd.ip_adapter import random_state_dict as ip_random
    from sid_lsg_amd.unet import CONFIGS as HC, random_state_dict
    usd = random_state_dict(HC[cfg_name], unet_seed) if usd is None else {k: v.detach().cpu() for k, v in usd.items()}
    unet = ControlledUNetRef(CONFIGS[cfg_name])
    unet.load_state_dict({k: usd[k] for k in unet.state_dict()})
    unet = unet.to(dtype).eval().requires_grad_(False)
    isd = ip_random(HC[cfg_name], EMBED_DIM, adapter_seed, TOKENS)
    ad = IPAdapterRef(unet).to(dtype)
    unet.to(dtype)                      # the wrapped attn2 modules (and their to_k_ip / to_v_ip) are the UNet's children
    ad.load_published(isd)
    ad.eval().requires_grad_(False)
    unet.eval().requires_grad_(False)
    return unet, ad, usd, isd


def make_inputs(cfg_name, B=3, h=8, w=16, seed=0):
    """x [B, 4, h, w], distinct timesteps [B], ctx [B, L, D] (bf16-representable), image embeddings [B, E] fp32."""
    cfg = CONFIGS[cfg_name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, h, w, generator=g).to(torch.bfloat16).float()
    t = torch.tensor([625, 37, 981, 250, 4][:B])
    ctx = torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g).to(torch.bfloat16).float()
    emb = torch.randn(B, EMBED_DIM, generator=g).to(torch.bfloat16).float()
    return x, t, ctx, emb


def ref_outputs(unet, ad, x, t, ctx, emb, scale=1.0, residuals=None):
    """fp64: (plain UNet output, image-prompted UNet output) [B, 4, h, w]; `residuals` = (down, mid) of a ControlNet for both."""
    d = next(unet.parameters()).dtype
    x, ctx = x.to(d), ctx.to(d)
    kw = {} if residuals is None else dict(down_residuals=residuals[0], mid_residual=residuals[1])
    with torch.no_grad():
        ad.set(None)
        plain = unet(x, t, encoder_hidden_states=ctx, **kw).sample
        ad.set(ad.image_proj(emb.to(d)), scale)
        out = unet(x, t, encoder_hidden_states=ctx, **kw).sample
        ad.set(None)
    return plain, out
