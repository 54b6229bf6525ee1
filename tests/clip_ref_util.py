"""Shared by tests/test_clip_host.py and tests/test_gpu_clip.py (not a test module): the CLIP golden file written out as a directory in
the Hugging Face layout, and the fp64 restatement of the reference wrapper's preprocessing (networks/clip.py:33-37)."""
import json
import os

import numpy as np
import torch

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)

# the resize cases of the clip_patches tests: (name, B, H, W, R, P)
RESIZE_CASES = (
    ('up_20_to_32', 3, 20, 20, 32, 8),            # upscale: the border clamp acts on all four sides
    ('down_40_to_28', 3, 40, 40, 28, 14),         # non-integer downscale: taps skip pixels; K = 588 is padded to 592
    ('rect_24x40_to_32', 3, 24, 40, 32, 8),       # H != W
    ('identity_32', 3, 32, 32, 32, 8),            # exactly (p / 255 - mean) / std up to one rounding
    ('prod_256_to_224', 1, 256, 256, 224, 14),    # the production ratio
)


def case_images(name, B, H, W):
    g = torch.Generator().manual_seed(sum(name.encode()))
    img = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    img[0, :, :2, :2] = 0             # pixels 0 and 255, in the corners where the clamp acts
    img[0, :, -2:, -2:] = 255
    img[-1, :, :2, -2:] = 255
    img[-1, :, -2:, :2] = 0
    return img


def _taps64(out, inp):
    """[out, 4] clamped tap indices and [out, 4] fp64 weights of F.interpolate(mode='bicubic', align_corners=False): A = -0.75,
    source coordinate (dst + 0.5) * in / out - 0.5, no antialiasing.  The COORDINATE is formed in fp32, as aten forms it
    (area_pixel_compute_scale / _source_index on float): it is part of the function -- at in = 256 an fp32 coordinate is 1.5e-5
    away from the real one, which moves a result by more than all the arithmetic behind it.  Weights and sums are fp64."""
    A = -0.75
    scale = torch.tensor(inp, dtype=torch.float32) / torch.tensor(out, dtype=torch.float32)
    src = scale * (torch.arange(out, dtype=torch.float32) + 0.5) - 0.5
    fl = torch.floor(src)
    t = (src - fl).double()                                              # exact in fp32
    inner = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1                 # noqa: E731   |x| <= 1
    outer = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A           # noqa: E731   1 < |x| < 2
    w = torch.stack([outer(t + 1), inner(t), inner(1 - t), outer(2 - t)], 1)
    idx = (fl.long()[:, None] + torch.arange(-1, 3)[None]).clamp(0, inp - 1)
    return idx, w


def pixel_values64(images_u8, R):
    """fp64 restatement: x / 255, bicubic to R x R (overshoot kept), (v - mean) / std.  -> [B, 3, R, R] fp64."""
    x = images_u8.to(torch.float64) / 255.0
    H, W = x.shape[-2:]
    iy, wy = _taps64(R, H)
    ix, wx = _taps64(R, W)
    rows = (x[:, :, iy, :] * wy[None, None, :, :, None]).sum(3)                   # [B, 3, R, W]
    v = (rows[:, :, :, ix] * wx[None, None, None, :, :]).sum(4)                   # [B, 3, R, R]
    mean, std = (torch.tensor(c, dtype=torch.float64).view(1, 3, 1, 1) for c in (MEAN, STD))
    return (v - mean) / std


def patch_rows64(pix, P):
    """[B, 3, R, R] -> [B, (R/P)^2, 3*P*P]: `unfold`, i.e. row gy * G + gx, column (c * P + py) * P + px."""
    return torch.nn.functional.unfold(pix, kernel_size=P, stride=P).transpose(1, 2)


VOCAB_WORDS = (['!'] + [chr(97 + i) for i in range(26)] + [chr(97 + i) + '</w>' for i in range(26)] + [f'{i}</w>' for i in range(9)]
               + ['<|startoftext|>', '<|endoftext|>'])          # 64 entries; BOS 62, EOS 63 as in the golden models


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'clip_ref.npz'))


def state_dict_of(ref, tag):
    pre = f'{tag}/sd/'
    return {k[len(pre):]: torch.from_numpy(ref[k]) for k in ref.files if k.startswith(pre)}


def write_clip_dir(ref, tag, dst, config_edit=None, drop=()):
    """Model `tag` of the golden file as a CLIP directory: config.json, model.safetensors, vocab.json, merges.txt."""
    from safetensors.torch import save_file
    os.makedirs(dst, exist_ok=True)
    cfg = json.loads(str(ref[f'{tag}/config']))
    if config_edit:
        config_edit(cfg)
    with open(os.path.join(dst, 'config.json'), 'w') as f:
        json.dump(cfg, f)
    save_file({k: v.contiguous() for k, v in state_dict_of(ref, tag).items() if k not in drop}, os.path.join(dst, 'model.safetensors'))
    with open(os.path.join(dst, 'vocab.json'), 'w') as f:
        json.dump({w: i for i, w in enumerate(VOCAB_WORDS)}, f)
    with open(os.path.join(dst, 'merges.txt'), 'w') as f:
        f.write('#version: 0.2\n')
    return str(dst)
