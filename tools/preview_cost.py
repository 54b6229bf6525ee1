#!/usr/bin/env python
"""Cost of one snapshot preview tick at the bench configuration: SD1.5 (random init), 512^2, batch_gpu 8 -- three 7 x 4 grids (1, 2 and 4
generation steps) rendered and written as PNG, as training_loop(snapshot_images=True) does at a snapshot tick.
    python tools/preview_cost.py [OUT_DIR]
Prints the wall time of a warm-up tick and of two timed ticks (host clock around work that ends in a device-to-host copy), split into
rendering and PNG encoding, and the grid kernel alone (device events around 100 calls on a decoded batch of 8 and of 28).  Under
`rocprofv3 --kernel-trace --stats -- python tools/preview_cost.py` the kernel's own rows are image_grid_u8_kernel<...>."""
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import ops, preview  # noqa: E402
from sid_lsg_amd.sd_util import load_sd15  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp()
os.makedirs(out_dir, exist_ok=True)
dev, res, batch_gpu = torch.device('cuda:0'), 512, 8
G, vae, sched, te, tok = load_sd15('random:sd15', None, dev, torch.bfloat16)
G.eval().requires_grad_(False)


class Prompts:
    def __len__(self):
        return 4096

    def __getitem__(self, i):
        return None, f'a photo of object number {i} on a table, studio light, {i % 7} colours'


grid = preview.setup_snapshot_grid(Prompts(), res, batch_gpu, (4, res // 8, res // 8), dev)
kw = dict(noise_scheduler=sched, text_encoder=te, tokenizer=tok, vae=vae, init_timestep=625, resolution=res)
for rep in range(3):
    t_render = t_png = 0.0
    for n in preview.STEP_COUNTS:
        torch.cuda.synchronize()
        t0 = time.time()
        img = preview.render_grid(G, grid, n, **kw).cpu().numpy()
        t1 = time.time()
        preview.save_png(os.path.join(out_dir, f'grid_{n}.png'), img)
        t_render, t_png = t_render + t1 - t0, t_png + time.time() - t1
    print(f'preview tick {"warm-up" if rep == 0 else rep}: {t_render + t_png:.2f} s = render (1 + 2 + 4 generator forwards and 3 decodes of 28 images, '
          f'device-to-host copy) {t_render:.2f} s + PNG encoding {t_png:.2f} s', flush=True)

out = torch.zeros((4 * res, 7 * res, 3), dtype=torch.uint8, device=dev)
for b in (8, 28):
    y = torch.randn(b, res, res, 8, device=dev)
    for layout, src in (('nhwc8', y), ('nchw', y[..., :3].permute(0, 3, 1, 2).contiguous())):
        for _ in range(5):
            ops.image_grid_u8(src, out, 0, 7, layout=layout)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            ops.image_grid_u8(src, out, 0, 7, layout=layout)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 10
        gb = (src.numel() * 4 * (0.5 if layout == 'nhwc8' else 1) + b * res * res * 3) / 1e9
        print(f'grid kernel, {b} images {layout}: {us:.1f} us per call (100 back-to-back calls; {gb / us * 1e6:.0f} GB/s of the bytes it needs)', flush=True)
