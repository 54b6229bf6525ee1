"""Write tests/golden/hps_ref.npz: Pillow's own results of open_clip's validation transform, and a seeded random-init CLIP model
evaluated by transformers.CLIPModel on the CPU in fp32 on them, stored under open_clip's key names.

    python tools/make_hps_goldens.py

PIL and transformers are needed HERE only: no test needs them (tests/test_hps_host.py compares with live Pillow when it imports).
Per preprocessing case `<name>` (CASES: source H x W, target R, patch P, what it covers):
  src/<name>   uint8 [B, 3, H, W] source images: all-0 and all-255 blocks next to noise (overshoot and clamping), single extreme pixels
  pil/<name>   uint8 [B, 3, R, R]: `Image.resize((w, h), BICUBIC)` with torchvision's Resize(R) size rule, then CenterCrop(R)
  pix/<name>   fp32 [B, 3, R, R]: ToTensor + Normalize by their torch lines (`x.float().div(255)`, `.sub_(mean).div_(std)`); the
               512 x 512 case leaves it out to stay small: both lines are element-wise, so it is norm_table[c][pil]
  norm_table   fp32 [3, 256]: those torch lines on every uint8 value
The model: image 32, patch 8, width 64, 2 heads, 2 layers, exact GELU, projection 32; text width 64, 2 heads, 2 layers, 64-token
vocabulary (BOS 62, EOS 63), 16 positions; every value rounded to a bf16-representable fp32 number.
  oc/<key>     the state dict RENAMED TO open_clip's LAYOUT: visual.conv1 / class_embedding / positional_embedding / ln_pre / ln_post,
               visual.proj and text_projection transposed, resblocks.N.attn.in_proj_{weight,bias} fused from q / k / v, attn.out_proj,
               ln_1 / ln_2, mlp.c_fc / c_proj, token_embedding, positional_embedding, ln_final, logit_scale
  ids          3 token rows (EOS at positions 3, 8, 15), padded with 0 behind EOS as open_clip's tokenizer pads
  image_embeds / text_embeds   CLIPModel's outputs (L2-normalised) on pix/down_40 and ids;  cosines: their row dot products
"""
import os

import numpy as np
import torch

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
BOS, EOS, VOCAB, MAX_POS = 62, 63, 64, 16

# name, B, H, W, R, P
CASES = [
    ('down_40', 3, 40, 40, 32, 8),          # down-scaling, windows clipped at both borders
    ('up_24', 2, 24, 24, 32, 8),            # up-scaling
    ('same_32', 2, 32, 32, 32, 8),          # no pass at all
    ('tall_64x48', 2, 64, 48, 32, 8),       # non-square, crop offset
    ('wide_48x64', 2, 48, 64, 32, 8),       # non-square, other orientation
    ('wide_64x74', 2, 64, 74, 32, 8),       # long side 37, crop remainder 2.5 -> 2, half to even
    ('wide_64x86', 2, 64, 86, 32, 8),       # long side 43, crop remainder 5.5 -> 6
    ('p14_24x40', 2, 24, 40, 28, 14),       # K = 588 padded to 592
    ('prod_512', 2, 512, 512, 224, 14),     # the production shape
]
NO_PIX = ('prod_512',)

VISION = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=32, patch_size=8,
              hidden_act='gelu', layer_norm_eps=1e-5)
TEXT = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, hidden_act='gelu', layer_norm_eps=1e-5)


def source_images(name, B, H, W, g):
    if name == 'prod_512':
        # structured, so that the file stays small: gradients, 0 / 255 blocks and stripes, noise in one corner only
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        img = np.zeros((B, 3, H, W), dtype=np.uint8)
        for b in range(B):
            for c in range(3):
                img[b, c] = ((xx * (c + 1) + yy * (3 - c) * (b + 1)) // 3) % 256
            img[b, :, 64:192, 64:192] = np.where(((yy[64:192, 64:192] // (16 + 5 * b)) + (xx[64:192, 64:192] // 11)) % 2, 255, 0)
            img[b, :, 300:400, :] = np.where((xx[300:400] % (3 + b)) == 0, 255, 0)          # stripes finer than the output grid
            img[b, :, -96:, -96:] = torch.randint(0, 256, (3, 96, 96), generator=g, dtype=torch.uint8).numpy()
            img[b, :, :40, -40:] = 255 * b
        return img
    img = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8).numpy()
    img[0, :, :H // 3, :W // 2] = 0
    img[0, :, H // 3:2 * H // 3, :W // 2] = 255
    img[1, :, -(H // 4):, -(W // 3):] = 255
    img[1, :, -(H // 2):-(H // 4), -(W // 3):] = 0
    img[-1, 0, 0, 0], img[-1, 1, -1, -1] = 255, 0
    return img


def pillow_transform(img, R):
    """torchvision's Resize(R, BICUBIC) + CenterCrop(R) on PIL images, by their own rules."""
    from PIL import Image
    B, _, H, W = img.shape
    h, w = (R, int(R * W / H)) if H <= W else (int(R * H / W), R)
    top, left = int(round((h - R) / 2.0)), int(round((w - R) / 2.0))
    out = []
    for b in range(B):
        im = Image.fromarray(np.ascontiguousarray(img[b].transpose(1, 2, 0)), 'RGB').resize((w, h), Image.BICUBIC)
        out.append(np.asarray(im.crop((left, top, left + R, top + R))).transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out))


def to_tensor_normalize(u8):
    """ToTensor (`.to(float32).div(255)`) and Normalize (`.sub_(mean).div_(std)`) on uint8 [..., 3, h, w]."""
    x = torch.from_numpy(u8).to(torch.float32).div(255)
    mean, std = torch.as_tensor(MEAN, dtype=torch.float32).view(3, 1, 1), torch.as_tensor(STD, dtype=torch.float32).view(3, 1, 1)
    return x.sub_(mean).div_(std)


def to_open_clip(sd):
    """A transformers CLIPModel state dict -> open_clip's names and layout."""
    out = {'logit_scale': sd['logit_scale'],
           'visual.conv1.weight': sd['vision_model.embeddings.patch_embedding.weight'],
           'visual.class_embedding': sd['vision_model.embeddings.class_embedding'],
           'visual.positional_embedding': sd['vision_model.embeddings.position_embedding.weight'],
           'visual.proj': sd['visual_projection.weight'].t().contiguous(),
           'text_projection': sd['text_projection.weight'].t().contiguous(),
           'token_embedding.weight': sd['text_model.embeddings.token_embedding.weight'],
           'positional_embedding': sd['text_model.embeddings.position_embedding.weight']}
    for p in ('weight', 'bias'):
        out[f'visual.ln_pre.{p}'] = sd[f'vision_model.pre_layrnorm.{p}']
        out[f'visual.ln_post.{p}'] = sd[f'vision_model.post_layernorm.{p}']
        out[f'ln_final.{p}'] = sd[f'text_model.final_layer_norm.{p}']
    for src, dst, n in (('vision_model.encoder.layers.', 'visual.transformer.resblocks.', VISION['num_hidden_layers']),
                        ('text_model.encoder.layers.', 'transformer.resblocks.', TEXT['num_hidden_layers'])):
        for i in range(n):
            for p in ('weight', 'bias'):
                out[f'{dst}{i}.attn.in_proj_{p}'] = torch.cat([sd[f'{src}{i}.self_attn.{x}_proj.{p}'] for x in 'qkv'])
                for hf, oc in (('self_attn.out_proj', 'attn.out_proj'), ('layer_norm1', 'ln_1'), ('layer_norm2', 'ln_2'), ('mlp.fc1', 'mlp.c_fc'),
                               ('mlp.fc2', 'mlp.c_proj')):
                    out[f'{dst}{i}.{oc}.{p}'] = sd[f'{src}{i}.{hf}.{p}']
    return out


def token_rows(g):
    """3 rows: BOS, 2 / 7 / 14 content tokens, EOS (positions 3, 8, 15), then zeros."""
    rows = []
    for n in (2, 7, MAX_POS - 2):
        body = [BOS] + torch.randint(1, BOS, (n,), generator=g).tolist() + [EOS]
        rows.append(body + [0] * (MAX_POS - len(body)))
    return torch.tensor(rows)


def main():
    from transformers import CLIPConfig, CLIPModel
    out = {}
    g = torch.Generator().manual_seed(2024)
    for name, B, H, W, R, P in CASES:
        src = source_images(name, B, H, W, g)
        pil = pillow_transform(src, R)
        out[f'src/{name}'], out[f'pil/{name}'] = src, pil
        if name not in NO_PIX:
            out[f'pix/{name}'] = to_tensor_normalize(pil).numpy()
        print(name, 'pil range', int(pil.min()), int(pil.max()), 'share at the clamps', float(((pil == 0) | (pil == 255)).mean()))
    out['norm_table'] = to_tensor_normalize(np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(1, 256), (3, 256)).reshape(3, 1, 256).copy()).reshape(3, 256).numpy()

    torch.manual_seed(300)
    text_config = dict(TEXT, vocab_size=VOCAB, max_position_embeddings=MAX_POS, bos_token_id=BOS, eos_token_id=EOS, pad_token_id=0)
    model = CLIPModel(CLIPConfig(vision_config=VISION, text_config=text_config, projection_dim=32)).eval().requires_grad_(False)
    with torch.no_grad():
        for pname, p in model.named_parameters():
            if p.dim() == 1:        # biases, norms, class embedding: not at their 0 / 1 start, which would hide a swapped or dropped one
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if 'norm' in pname and pname.endswith('weight') else 0.0))
            elif 'embedding' in pname:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif p.dim() == 0:
                continue
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 * p.shape[1] ** -0.5 if p.dim() == 2 else 0.1))
            p.copy_(p.to(torch.bfloat16).float())
    ids = token_rows(g)
    pix = torch.from_numpy(out['pix/down_40'])
    with torch.no_grad():
        o = model(input_ids=ids, pixel_values=pix)
    sd = {k: v.float() for k, v in model.state_dict().items() if not k.endswith('position_ids')}
    for k, v in to_open_clip(sd).items():
        out[f'oc/{k}'] = v.numpy()
    out['ids'] = ids.numpy()
    out['image_embeds'], out['text_embeds'] = o.image_embeds.float().numpy(), o.text_embeds.float().numpy()
    out['cosines'] = (o.image_embeds * o.text_embeds).sum(-1).float().numpy()
    print('cosines', out['cosines'], 'params', sum(p.numel() for p in model.parameters()))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'hps_ref.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
