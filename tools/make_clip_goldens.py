"""Write tests/golden/clip_ref.npz: two seeded random-init CLIP models evaluated by transformers.CLIPModel on the CPU in fp32.

    python tools/make_clip_goldens.py

transformers is needed HERE only: no test imports it.  Per model (prefix `a/` and `b/`) the file holds
  config            the config.json text (vision_config / text_config / projection_dim)
  sd/<key>          the state dict under the transformers key names, every value rounded to a bf16-representable fp32 number (the
                    bf16 compute mode then carries no weight-rounding term, and the file compresses)
  images            3 uint8 source images [3, 3, H, W], pixels 0 and 255 included
  ids_pad0 / ids_padeos   the same 3 token rows (EOS at different positions), padded behind EOS with 0 / with EOS
  pixel_values      the reference wrapper's preprocessing (networks/clip.py:33-37) by its own torch lines on the CPU
  image_embeds / text_embeds   CLIPModel's outputs (L2-normalised), fp32;  cosines: their row dot products
Model (a): image 32, patch 8, width 64, 2 heads, 2 layers, quick_gelu, projection 32; images 40 x 40.
Model (b): image 28, patch 14 (K = 588, padded to 592), width 88, 1 head (head dim 88, ViT-g's), 2 layers, gelu, projection 24; images 24 x 40.
Both: 64-token vocabulary (BOS 62, EOS 63), 16 text positions.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
BOS, EOS, VOCAB, MAX_POS = 62, 63, 64, 16

MODELS = {
    'a': dict(projection_dim=32, src=(40, 40),
              vision_config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=32, patch_size=8,
                                 hidden_act='quick_gelu', layer_norm_eps=1e-5),
              text_config=dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, hidden_act='quick_gelu',
                               layer_norm_eps=1e-5)),
    'b': dict(projection_dim=24, src=(24, 40),
              vision_config=dict(hidden_size=88, intermediate_size=176, num_hidden_layers=2, num_attention_heads=1, image_size=28, patch_size=14,
                                 hidden_act='gelu', layer_norm_eps=1e-5),
              text_config=dict(hidden_size=48, intermediate_size=96, num_hidden_layers=2, num_attention_heads=2, hidden_act='gelu',
                               layer_norm_eps=1e-5)),
}


def token_rows(g):
    """3 rows: BOS, 2 / 7 / 14 content tokens, EOS (positions 3, 8, 15), then padding."""
    rows0, rows1 = [], []
    for n in (2, 7, MAX_POS - 2):
        body = [BOS] + torch.randint(1, BOS, (n,), generator=g).tolist() + [EOS]
        rows0.append(body + [0] * (MAX_POS - len(body)))
        rows1.append(body + [EOS] * (MAX_POS - len(body)))
    return torch.tensor(rows0), torch.tensor(rows1)


def main():
    from transformers import CLIPConfig, CLIPModel
    out = {}
    for seed, (tag, m) in enumerate(MODELS.items()):
        torch.manual_seed(100 + seed)
        text_config = dict(m['text_config'], vocab_size=VOCAB, max_position_embeddings=MAX_POS, bos_token_id=BOS, eos_token_id=EOS, pad_token_id=0)
        cfg = dict(vision_config=m['vision_config'], text_config=text_config, projection_dim=m['projection_dim'])
        model = CLIPModel(CLIPConfig(**cfg)).eval().requires_grad_(False)
        g = torch.Generator().manual_seed(200 + seed)
        with torch.no_grad():
            for name, p in model.named_parameters():
                if p.dim() == 1:        # biases, norms and the class embedding: transformers starts them at 0 / 1, which would hide a swapped or dropped one
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if 'norm' in name and name.endswith('weight') else 0.0))
                elif 'embedding' in name:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.3)
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * (2.0 * p.shape[1] ** -0.5 if p.dim() == 2 else 0.1))
                p.copy_(p.to(torch.bfloat16).float())
        H, W = m['src']
        images = torch.randint(0, 256, (3, 3, H, W), generator=g, dtype=torch.uint8)
        images[0, :, :2, :3] = 0
        images[1, :, -2:, -3:] = 255
        images[2, 0, 0, 0], images[2, 1, -1, -1] = 255, 0
        R = m['vision_config']['image_size']
        pix = F.interpolate(images.to(torch.float32) / 255., R, mode='bicubic', align_corners=False)
        pix = (pix - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
        ids0, ids1 = token_rows(g)
        with torch.no_grad():
            o = model(input_ids=ids1, pixel_values=pix)
            o0 = model(input_ids=ids0, pixel_values=pix)
        assert float((o.text_embeds - o0.text_embeds).abs().max()) < 1e-6, 'padding behind EOS changed the pooled text embedding'
        out[f'{tag}/config'] = np.array(json.dumps(cfg))
        for k, v in model.state_dict().items():
            if k == 'logit_scale' or k.endswith('position_ids'):
                continue
            out[f'{tag}/sd/{k}'] = v.float().numpy()
        out[f'{tag}/images'] = images.numpy()
        out[f'{tag}/ids_pad0'], out[f'{tag}/ids_padeos'] = ids0.numpy(), ids1.numpy()
        out[f'{tag}/pixel_values'] = pix.numpy()
        out[f'{tag}/image_embeds'], out[f'{tag}/text_embeds'] = o.image_embeds.float().numpy(), o.text_embeds.float().numpy()
        out[f'{tag}/cosines'] = (o.image_embeds * o.text_embeds).sum(-1).float().numpy()
        print(tag, 'cosines', out[f'{tag}/cosines'], 'params', sum(p.numel() for p in model.parameters()))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'clip_ref.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
