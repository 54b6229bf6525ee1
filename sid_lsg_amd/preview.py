"""Snapshot preview grids: the `fakes_init.png` / `fakes_<alpha>_<kimg>_<n>.png` pictures the reference's loop writes at start-up and
at every snapshot tick (training/sid_training_loop.py:39-50 setup_snapshot_image_grid, :53-70 split_list, :99-115 save_image_grid,
:258-271, :347-364, :597-616) and the `<metric><kimg>_<n>.png` grids of its evaluation branch (:704-733).

  * setup_snapshot_grid: which prompts and which latents fill the grid.  gw x gh = clip(3840 // res, 7, 32) x clip(2160 // res, 4, 32)
    tiles (7 x 4 at 512 and 768, 15 x 8 at 256), prompts by numpy.random.RandomState(0).shuffle of the dataset's indices, taken
    cyclically, in chunks of batch_gpu.  grid_z comes from a PRIVATE torch.Generator seeded 2024: the reference seeds the global
    generator with 2024 and re-seeds it afterwards; a private one leaves the training noise untouched, previews on or off.
  * render_grid: G (the EMA generator) through sid_sd_sampler's evaluation sampler with n generation steps, chunk by chunk, each
    chunk decoded straight into its tiles of a uint8 grid on the device (HipAutoencoderKLDecoder.decode_to_grid ->
    sidlsg_image_grid_u8).  The sampler's steps 2 .. n draw noise from the device's global generator; render_grid runs under a
    forked generator state seeded per call, so a grid depends on (weights, n) alone and the caller's RNG stream does not see it.
  * save_png: PIL when present, else a zlib + CRC writer.

  * write_sampled_grid: one grid through any deterministic latent sampler (the teacher's DDIM sampler: `<metric>_teacher.png`).

  * write_reals: `reals.png` (sid_training_loop.py:347-350), when the dataset yields pixels (data.ImageCaptionDataset): the first
    gw x gh items of the set, taken cyclically, in range 0..255 through the same grid kernel.
"""
import os
import struct
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from .sd_util import sid_sd_sampler

GRID_SEED = 2024
STEP_COUNTS = (1, 2, 4)         # generation steps of the grids of one snapshot (sid_training_loop.py:601, 723)


def grid_layout(num_items, resolution):
    """-> (gw, gh), [dataset index of every tile]   (setup_snapshot_image_grid with its default random_seed=0)"""
    gw = int(np.clip(3840 // resolution, 7, 32))
    gh = int(np.clip(2160 // resolution, 4, 32))
    order = list(range(num_items))
    np.random.RandomState(0).shuffle(order)
    return (gw, gh), [order[i % num_items] for i in range(gw * gh)]


def split_chunks(items, size):
    """Chunks of `size` items, the last one shorter (split_list with an integer size)."""
    return [list(items[i:i + size]) for i in range(0, len(items), size)]


def setup_snapshot_grid(dataset, resolution, batch_gpu, latent_shape, device):
    """-> namespace(size=(gw, gh), indices, z=[chunks of [b, *latent_shape] fp32 on device], c=[chunks of prompts])"""
    size, indices = grid_layout(len(dataset), resolution)
    contexts = [dataset[i][1] for i in indices]
    gen = torch.Generator(device).manual_seed(GRID_SEED)
    z = torch.randn([len(contexts), *latent_shape], device=device, dtype=torch.float32, generator=gen)
    return SimpleNamespace(size=size, indices=indices, z=list(z.split(batch_gpu)), c=split_chunks(contexts, batch_gpu))


def render_grid(G, grid, num_steps_eval, *, noise_scheduler, text_encoder, tokenizer, vae, init_timestep, resolution, num_steps=1):
    """-> uint8 [gh * resolution, gw * resolution, 3] on the device: tile i = image of (grid_z[i], prompt i), drange [-1, 1]."""
    device = grid.z[0].device
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('render_grid inside a graph capture: the preview is never part of a captured step')
    gw, gh = grid.size
    out = torch.zeros((gh * resolution, gw * resolution, 3), dtype=torch.uint8, device=device)
    with torch.no_grad(), torch.random.fork_rng(devices=[device]), torch.cuda.device(device):
        torch.cuda.manual_seed(GRID_SEED)
        first = 0
        for z, c in zip(grid.z, grid.c):
            x = sid_sd_sampler(unet=G, latents=z, contexts=c, init_timesteps=init_timestep * torch.ones((len(c),), device=device, dtype=torch.long),
                               noise_scheduler=noise_scheduler, text_encoder=text_encoder, tokenizer=tokenizer, resolution=resolution,
                               dtype=torch.float32, return_images=False, num_steps=num_steps, train_sampler=False,
                               num_steps_eval=num_steps_eval)
            vae.decode_to_grid(x.to(vae.dtype) / vae.config.scaling_factor, out, first, gw)
            first += len(c)
    return out


def write_sampled_grid(path, grid, resolution, vae, sample):
    """One PNG of the grid's (z, prompts) chunks through `sample(z, prompts) -> latents fp32 NCHW` (a deterministic sampler that draws
    no noise, e.g. sd_util.teacher_sample), decoded straight into the tiles by the grid kernel as render_grid does."""
    device = grid.z[0].device
    gw, gh = grid.size
    out = torch.zeros((gh * resolution, gw * resolution, 3), dtype=torch.uint8, device=device)
    with torch.no_grad(), torch.cuda.device(device):
        first = 0
        for z, c in zip(grid.z, grid.c):
            x = sample(z, c)
            vae.decode_to_grid(x.to(vae.dtype) / vae.config.scaling_factor, out, first, gw)
            first += len(c)
    save_png(path, out.cpu().numpy())
    return path


def write_reals(out_dir, dataset, size, resolution, device):
    """<out_dir>/reals.png: item i % len(dataset) in tile i.  The images are shown as stored, so they must be resolution x resolution."""
    from . import ops
    gw, gh = size
    out = torch.zeros((gh * resolution, gw * resolution, 3), dtype=torch.uint8, device=device)
    for i in range(gw * gh):
        image = dataset[i % len(dataset)][0]
        if tuple(image.shape[-2:]) != (resolution, resolution):
            raise ValueError(f'reals.png: item {i % len(dataset)} is {tuple(image.shape[-2:])}, the grid needs {resolution} x {resolution} images')
        if image.shape[0] == 1:
            image = image.repeat(3, 1, 1)
        ops.image_grid_u8(image[None].to(device, torch.float32).contiguous(), out, i, gw, drange=(0, 255), layout='nchw')
    path = os.path.join(out_dir, 'reals.png')
    save_png(path, out.cpu().numpy())
    return path


def write_grids(out_dir, name_format, G, grid, step_counts=STEP_COUNTS, **render_kwargs):
    """One PNG per step count n: <out_dir>/<name_format.format(n=n)>.  Each ends in a device-to-host copy, i.e. synchronises the stream."""
    paths = []
    for n in step_counts:
        img = render_grid(G, grid, n, **render_kwargs)
        paths.append(os.path.join(out_dir, name_format.format(n=n)))
        save_png(paths[-1], img.cpu().numpy())
    return paths


def png_bytes(hwc_uint8):
    """A minimal RGB8 PNG (zlib + CRC, one IDAT)."""
    h, w, _ = hwc_uint8.shape
    raw = b''.join(b'\x00' + hwc_uint8[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def save_png(path, hwc_uint8):
    try:
        import PIL.Image
        PIL.Image.fromarray(hwc_uint8, 'RGB').save(path)
    except ImportError:                    # no Pillow: the minimal writer is enough for RGB8
        with open(path, 'wb') as f:
            f.write(png_bytes(hwc_uint8))
