"""Shared by tests/test_hps_host.py and tests/test_gpu_hps.py: the golden file of tools/make_hps_goldens.py and the files the HPSv2
scorer reads (a checkpoint in open_clip's layout, tokenizer files, benchmark prompt lists), written from it."""
import json
import os

import numpy as np
import torch

from clip_ref_util import MEAN, STD, VOCAB_WORDS  # noqa: F401

# name, B, H, W, R, P: tools/make_hps_goldens.py CASES
CASES = (
    ('down_40', 3, 40, 40, 32, 8),
    ('up_24', 2, 24, 24, 32, 8),
    ('same_32', 2, 32, 32, 32, 8),
    ('tall_64x48', 2, 64, 48, 32, 8),
    ('wide_48x64', 2, 48, 64, 32, 8),
    ('wide_64x74', 2, 64, 74, 32, 8),
    ('wide_64x86', 2, 64, 86, 32, 8),
    ('p14_24x40', 2, 24, 40, 28, 14),
    ('prod_512', 2, 512, 512, 224, 14),
)
# resized (h, w) and crop (top, left) by torchvision's rules, worked out by hand: 32 * 74 / 64 = 37, (37 - 32) / 2 = 2.5 -> 2 (half to
# even); 32 * 86 / 64 = 43, 5.5 -> 6; 32 * 64 / 48 = 42.67 -> 42, 5; 28 * 40 / 24 = 46.67 -> 46, 9
GEOMETRY = {'down_40': ((32, 32), (0, 0)), 'up_24': ((32, 32), (0, 0)), 'same_32': ((32, 32), (0, 0)), 'tall_64x48': ((42, 32), (5, 0)),
            'wide_48x64': ((32, 42), (0, 5)), 'wide_64x74': ((32, 37), (0, 2)), 'wide_64x86': ((32, 43), (0, 6)),
            'p14_24x40': ((28, 46), (0, 9)), 'prod_512': ((224, 224), (0, 0))}
STYLES = ('anime', 'concept-art', 'paintings', 'photo')


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'hps_ref.npz'))


def pixel_values(ref, name):
    """fp32 [B, 3, R, R]: the stored torch ToTensor / Normalize result, or (the 512 x 512 case) the stored table of those element-wise
    lines looked up at the stored Pillow picture."""
    if f'pix/{name}' in ref.files:
        return torch.from_numpy(ref[f'pix/{name}'])
    table, pil = torch.from_numpy(ref['norm_table']), torch.from_numpy(ref[f'pil/{name}']).long()
    return torch.stack([table[c][pil[:, c]] for c in range(3)], 1)


def open_clip_state(ref):
    return {k[3:]: torch.from_numpy(ref[k]) for k in ref.files if k.startswith('oc/')}


def write_tokenizer(dst):
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, 'vocab.json'), 'w') as f:
        json.dump({w: i for i, w in enumerate(VOCAB_WORDS)}, f)
    with open(os.path.join(dst, 'merges.txt'), 'w') as f:
        f.write('#version: 0.2\n')
    return str(dst)


def write_checkpoint(ref, path, wrap=False):
    """The golden model as an open_clip checkpoint: `.safetensors` or torch.save; wrap: under `state_dict` with `module.` prefixes."""
    sd = {k: v.contiguous() for k, v in open_clip_state(ref).items()}
    if str(path).endswith('.safetensors'):
        from safetensors.torch import save_file
        save_file(sd, str(path))
    else:
        torch.save({'state_dict': {'module.' + k: v for k, v in sd.items()}, 'epoch': 3} if wrap else sd, str(path))
    return str(path)


def write_prompts(dst, n):
    """n prompts per style from the letters and digits of the test vocabulary."""
    os.makedirs(dst, exist_ok=True)
    words = ['a red cube', 'two cats on a hill', 'the sea at night', 'green field', 'blue sphere 3', 'an old house', 'x', 'dog 7 and bird']
    out = {}
    for j, style in enumerate(STYLES):
        out[style] = [f'{style.replace("-", " ")} {words[(i + j) % len(words)]} {i}' for i in range(n)]
        with open(os.path.join(dst, style + '.json'), 'w') as f:
            json.dump(out[style], f)
    return str(dst), out
