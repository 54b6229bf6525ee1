#!/usr/bin/env python
"""One-step text-to-image generation with a distilled generator (counterpart of the reference's `generate_onestep.py`).

    torchrun --standalone --nproc_per_node=8 generate_onestep.py --network runs/00000-.../network-snapshot-1.000000-000500.pkl \\
        --outdir out --seeds 0-63 --batch 16 --text_prompts prompts.txt --repo_id /models/stable-diffusion-v1-5

Same options and file layout as the reference (`generate_onestep.py:113-125, 218-311`): image i uses prompt line i and the
latent drawn from torch.Generator(seed_i) (`StackedRandomGenerator`), x_hat = G(z; t_init) in one UNet evaluation,
`vae.decode(x_hat / scaling_factor)`, uint8 `(img*127.5+128).clip(0,255)` PNG named `<seed:06d>.png`.  Batches are strided
over ranks.  `--repo_id` must be a local diffusers-layout directory (text encoder, tokenizer, VAE, scheduler) or `random:<arch>`
(`random:<arch>:v` for a v-prediction model); its parameterisation must be the snapshot's.  `--resolution` is the image size
(latent = resolution / 8; 768 for an SD 2.x 768-v generator).

`--init_images DIR` turns it into image-to-image generation: sample `idx` (the index that picks its prompt) starts from file
`idx % len(files)` of DIR (PNG / JPEG, sorted by name; centre-cropped to a square and resized to `--resolution`), encoded by the VAE
encoder on the HIP kernels (sid_lsg_amd.vae.HipAutoencoderKLEncoder) and re-noised with the sample's own z.  A generator trained with
`--num_steps N` is entered at step k of its chain, chosen by `--strength` (strength_to_step); for a one-step generator the knob is
`--init_timestep`.  Without `--init_images` nothing changes.

`--network teacher` samples the teacher itself instead of a snapshot: the UNet of `--repo_id` under classifier-free guidance
(`--guidance_scale`, default 7.5) and a deterministic DDIM sampler of `--teacher_steps` steps (default 50;
sid_lsg_amd.sd_util.teacher_sample), with the same seeds, prompts and file names -- the teacher row of the SiD-LSG tables.
`--teacher_sampler {ddim,dpmpp2m}`, `--teacher_spacing {leading,trailing,linspace}`, `--teacher_eta`, `--guidance_rescale` and
`--negative_prompt` choose the solver family of sd_util.teacher_sample_solver instead (DPM-Solver++ 2M, stochastic DDIM, 'trailing'
spacing with guidance rescale as SD 2.1 768-v is usually run); with none of them given the DDIM path above runs unchanged.
`--network teacher --init_images DIR --strength S` is image-to-image with the teacher, under every sampler option above: the chain of
`--teacher_steps` steps is entered at step k = N - min(int(N S), N) (sd_util.teacher_start_index, diffusers' rule) from the encoded
image noised to t_k with the sample's z.  `--strength` has no default here and must be given.

`--mask_images DIR` (with `--init_images`) is inpainting: one mask file, or one per init image (sorted by name; sample `idx` uses
file `idx % len`), white = repaint.  A mask gets the init image's centre crop and a NEAREST resize; a latent cell is repainted if any
pixel of its 8 x 8 block is >= 128, so everything marked is repainted (diffusers takes the nearest pixel).  The samplers re-impose the
kept region at every step boundary (sidlsg_masked_renoise).  `--mask_composite 1` also takes the pixels whose mask value is < 128
from the init image as loaded, after decoding: the VAE round trip alone changes kept pixels slightly.

`--controlnet SPEC --control_images DIR` conditions every UNet call on a ControlNet (sid_lsg_amd.controlnet.HipControlNet): SPEC is a
local directory in diffusers' layout or `random:controlnet[:seed]`; sample `idx` takes control image `idx % len(files)` of DIR (PNG /
JPEG, sorted by name), which must already be `--resolution` square -- an edge map or a pose skeleton is not resampled behind the user's
back.  `--control_scale` (default 1) scales the thirteen residuals.  It applies to `--network teacher` under every `--teacher_*` option
and to snapshots with any `--num_steps_eval`, and combines with `--init_images` / `--mask_images`.

`--ip_adapter SPEC --ip_image_encoder DIR --ip_images DIR` gives every sample a reference picture as an image prompt (IP-Adapter,
sid_lsg_amd.ip_adapter.HipIPAdapter): SPEC is a local `.safetensors` / `.bin` file of an SD 1.5 adapter with the linear image projection
or `random:ip-adapter[:seed]`; the image encoder is a local CLIP directory (config.json, model.safetensors) or `random:clip-<arch>`;
sample `idx` takes prompt image `idx % len(files)` of DIR, any size (the encoder's CLIPImageProcessor transform resizes).  `--ip_scale`
(default 1) scales the image attention; 0 issues exactly the launches of a run without the options.  It applies wherever `--controlnet`
does and combines with it.

`--lora SPEC` (repeatable) merges LoRA files into the UNet and the text encoder before sampling (sid_lsg_amd.lora.LoraSet: one merge launch
per network on the fp32 masters, then the usual refresh of the compute copies): SPEC is a local kohya / A1111 or diffusers / PEFT
`.safetensors` / `.bin` / `.pt` file, or `random:lora[:rank[:seed]]`.  `--lora_scale S` (repeatable: none = 1, one value for all files, or
one per file; negative allowed) scales them; 0 leaves weights equal (torch.equal) to those of a run without `--lora`.  The sampling loop is untouched, so it applies to
snapshots and to `--network teacher` under every option above, and a LoRA run issues exactly the launches of the plain run per step.

`--control_preprocess canny` makes the control images here: `--control_images` then holds photographs of any size, loaded by the rule
of load_init_image (centre crop, LANCZOS resize), and their Canny edge map (sid_lsg_amd.edges.canny: OpenCV's Canny(img, 100, 200), the
ControlNet annotator, on the device; `--canny_low` / `--canny_high`) is the hint.  `--control_adherence 1` scores every written image, as
the uint8 that goes into its PNG: the Canny edges of the output against the edge set of its control image (any channel >= 128; for a
preprocessed run the Canny map itself) -- precision, recall and F1 with `--edge_tolerance` pixels (default 1) -- into
`<outdir>/control_adherence.json` (`options`, `per_image` keyed by PNG name, `mean`, micro-averaged).  Without the options nothing changes.

`--fidelity 1` (with `--init_images`) compares every written image, as the uint8 that goes into its PNG, with the init image it started
from (the crop load_init_image produced) on the device: PSNR and SSIM (sid_lsg_amd.fidelity, sidlsg_psnr_ssim_u8), and LPIPS-VGG when
`--lpips_vgg SPEC --lpips_lin SPEC` name a torchvision VGG16 state dict and the lpips package's lin weights (or
`random:lpips-vgg[:seed]` for both).  With `--mask_images` the `_keep` figures are those of the kept region (mask < 128).  Rank 0 writes
`<outdir>/fidelity.json` (`options`, `per_image` keyed by PNG name, `mean`).  Without the option nothing changes.

`--seeds_per_prompt K` (default 1) draws K samples per condition: sample `idx` keeps its seed and its file name and takes condition
`idx // K` wherever `idx` selects one above (the prompt, the init image, the mask, the control image, the IP image).  `--diversity 1`
(with K >= 2, both `--lpips_*` specs and a sample count that is a multiple of K) then scores, after generation, how different the K
images of each prompt are (sid_lsg_amd.diversity): the LPIPS of all K (K - 1) / 2 pairs from ONE VGG16 pass over the K images
(sidlsg_lpips_group_f32, each value the bits the paired path gives), their mean and minimum, and the mean SSIM and MSE of the same
pairs.  Group g is scored by rank g mod world from the PNG files read back, so batch and rank boundaries do not matter.  Rank 0 writes
`<outdir>/diversity.json` (`options`, `per_prompt` keyed by group index with `prompt`, `files` and the figures, `mean`).
"""
import json
import math
import os
import pickle
import re
from types import SimpleNamespace
from typing import NamedTuple

import click
import numpy as np
import torch

from sid_lsg_amd import distributed as dist
from sid_lsg_amd import diversity as prompt_diversity
from sid_lsg_amd.clip import load_clip_vision
from sid_lsg_amd import edges as edge_maps
from sid_lsg_amd.fidelity import aggregate as aggregate_fidelity
from sid_lsg_amd.fidelity import check_specs as check_lpips_specs
from sid_lsg_amd.fidelity import format_means, load_lpips, score_batch
from sid_lsg_amd.preview import save_png
from sid_lsg_amd.sd_util import (TEACHER, TEACHER_CFG, TEACHER_STEPS, check_prediction_type, load_controlnet, load_ip_adapter, load_lora, load_sd15, load_vae_encoder, lora_scales,
                                 sid_sd_sampler, teacher_sample_i2i, teacher_sample_solver_i2i, teacher_start_index)


class StackedRandomGenerator:
    """One torch.Generator per sample, so that image i does not depend on the batch it is generated in."""

    def __init__(self, device, seeds):
        self.generators = [torch.Generator(device).manual_seed(int(s) % (1 << 32)) for s in seeds]

    def randn(self, size, **kw):
        assert size[0] == len(self.generators)
        return torch.stack([torch.randn(size[1:], generator=g, **kw) for g in self.generators])


def parse_int_list(s):
    """'1,2,5-10' -> [1, 2, 5, 6, 7, 8, 9, 10]"""
    if isinstance(s, list):
        return s
    out = []
    for part in s.split(','):
        m = re.fullmatch(r'(\d+)-(\d+)', part)
        out.extend(range(int(m.group(1)), int(m.group(2)) + 1) if m else [int(part)])
    return out


def read_prompts(path):
    with open(path, 'rt') as f:
        return [line.strip() for line in f if line.strip()]


# What the *_options functions below return (None when their options are not given): plain tuples with names, in the order of each docstring
TeacherOpt = NamedTuple('TeacherOpt', [('steps', int), ('guidance_scale', float)])
Img2ImgOpt = NamedTuple('Img2ImgOpt', [('files', list), ('start', int), ('sample_posterior', bool)])
MaskOpt = NamedTuple('MaskOpt', [('files', list), ('composite', bool)])
ControlOpt = NamedTuple('ControlOpt', [('spec', str), ('files', list), ('scale', float)])
EdgeOpt = NamedTuple('EdgeOpt', [('preprocess', bool), ('low', int), ('high', int), ('adherence', bool), ('tolerance', int)])
IpOpt = NamedTuple('IpOpt', [('adapter', str), ('image_encoder', str), ('files', list), ('scale', float)])
LoraOpt = NamedTuple('LoraOpt', [('specs', list), ('scales', list)])
FidelityOpt = NamedTuple('FidelityOpt', [('lpips_vgg', str), ('lpips_lin', str)])
DiversityOpt = NamedTuple('DiversityOpt', [('lpips_vgg', str), ('lpips_lin', str), ('groups', dict)])


def teacher_options(network_pkl, teacher_steps, guidance_scale):
    """-> (steps, guidance scale) when --network is the teacher sentinel, else None; the teacher's options with a snapshot are refused."""
    if network_pkl != TEACHER:
        given = [f for f, v in (('--teacher_steps', teacher_steps), ('--guidance_scale', guidance_scale)) if v is not None]
        if given:
            raise click.UsageError(f'{" / ".join(given)} apply to --network {TEACHER} only: a distilled generator is sampled without guidance '
                                   'in --num_steps_eval steps')
        return None
    return TeacherOpt(TEACHER_STEPS if teacher_steps is None else teacher_steps, TEACHER_CFG if guidance_scale is None else guidance_scale)


def teacher_solver_options(network_pkl, teacher_sampler=None, teacher_spacing=None, teacher_eta=None, guidance_rescale=None,
                           negative_prompt=None):
    """-> None when none of the solver options of --network teacher is given (the deterministic DDIM path of teacher_sample runs, as
    before they existed), else the keywords of sd_util.teacher_sample_solver except negative_contexts, plus the negative prompt; the
    options with a snapshot, and combinations the schedule refuses, are usage errors."""
    given = [f for f, v in (('--teacher_sampler', teacher_sampler), ('--teacher_spacing', teacher_spacing), ('--teacher_eta', teacher_eta),
                            ('--guidance_rescale', guidance_rescale), ('--negative_prompt', negative_prompt)) if v is not None]
    if not given:
        return None
    if network_pkl != TEACHER:
        raise click.UsageError(f'{" / ".join(given)} apply to --network {TEACHER} only')
    solver = 'ddim' if teacher_sampler is None else teacher_sampler
    if solver == 'dpmpp2m' and teacher_eta:
        raise click.UsageError(f'--teacher_eta {teacher_eta:g}: --teacher_sampler dpmpp2m is deterministic (eta applies to ddim)')
    if solver == 'ddim' and teacher_spacing == 'linspace':
        raise click.UsageError('--teacher_spacing linspace: not reproduced for --teacher_sampler ddim (use leading or trailing)')
    return dict(solver=solver, spacing=teacher_spacing, eta=0.0 if teacher_eta is None else float(teacher_eta),
                guidance_rescale=0.0 if guidance_rescale is None else float(guidance_rescale), negative_prompt=negative_prompt)


IMAGE_EXTENSIONS = ('.png', '.jpg', '.jpeg')


def strength_to_step(strength, num_steps):
    """--strength S in (0, 1] -> the step k at which an N-step generator's chain is entered: k = clamp(N - ceil(S N), 0, N - 1).
    S = 1 runs all N steps from the image re-noised at t_init (the most noise, the least of the image kept), a small S only the last
    step.  N = 4: 1 -> 0, 0.75 -> 1, 0.6 -> 1, 0.5 -> 2, 0.25 -> 3, 0.01 -> 3; N = 1: always 0."""
    if not 0 < strength <= 1:
        raise ValueError(f'strength {strength}: expected a value in (0, 1]')
    if num_steps < 1:
        raise ValueError(f'num_steps {num_steps}: expected at least one step')
    run = math.ceil(strength * num_steps - 1e-9)          # S N is formed in floating point: 0.3 * 10 must count as 3 steps, not 4
    return min(max(num_steps - run, 0), num_steps - 1)


def image_files(path, flag, expect=None):
    """The PNG / JPEG files of directory `path`, the value of option `flag`, sorted by name.  At least one, or with `expect` (the mask's
    rule) exactly 1 or `expect` of them."""
    if not os.path.isdir(path):
        raise click.UsageError(f'{flag} {path}: not a directory')
    files = sorted(f for f in os.listdir(path) if f.lower().endswith(IMAGE_EXTENSIONS) and os.path.isfile(os.path.join(path, f)))
    if expect is None and not files:
        raise click.UsageError(f'{flag} {path}: no PNG or JPEG files')
    if expect is not None and len(files) not in (1, expect):
        raise click.UsageError(f'{flag} {path}: {len(files)} PNG or JPEG files, expected 1 or one per init image ({expect})')
    return [os.path.join(path, f) for f in files]


def list_init_images(path):
    """The PNG / JPEG files of a directory, sorted by name."""
    return image_files(path, '--init_images')


def _load_square(path, resolution, mode, resample):
    """-> uint8 [resolution, resolution(, 3)]: converted to `mode`, centre-cropped to a square, resized with PIL's filter `resample`."""
    import PIL.Image
    with PIL.Image.open(path) as im:
        im = im.convert(mode)
        w, h = im.size
        side = min(w, h)
        left, top = (w - side) // 2, (h - side) // 2
        im = im.crop((left, top, left + side, top + side))
        if side != resolution:
            im = im.resize((resolution, resolution), getattr(PIL.Image, resample))
        return np.ascontiguousarray(np.asarray(im, dtype=np.uint8))


def _batch(load, files, indices, resolution):
    """Sample idx takes file idx % len(files) -> the stacked load(file, resolution)."""
    return np.stack([load(files[i % len(files)], resolution) for i in indices])


def load_init_image(path, resolution):
    """-> uint8 [resolution, resolution, 3]: RGB, centre-cropped to a square, resized with PIL's LANCZOS filter (on the host)."""
    return _load_square(path, resolution, 'RGB', 'LANCZOS')


def load_init_batch(files, indices, resolution):
    """Sample idx takes file idx % len(files) -> uint8 [B, resolution, resolution, 3]."""
    return _batch(load_init_image, files, indices, resolution)


def init_image_options(network_pkl, init_images, strength, sample_posterior, num_steps_eval):
    """-> None without --init_images, else (files, entry step k, sample the posterior?); inconsistent options are refused."""
    if init_images is None:
        given = [f for f, v in (('--strength', strength), ('--sample_posterior', sample_posterior)) if v is not None]
        if given:
            raise click.UsageError(f'{" / ".join(given)} apply to --init_images only')
        return None
    if network_pkl == TEACHER:
        raise click.UsageError(f'--init_images with --network {TEACHER}: image-to-image with the teacher sampler is not supported')
    if num_steps_eval < 1:
        raise click.UsageError('--init_images needs --num_steps_eval >= 1')
    files = list_init_images(init_images)
    return Img2ImgOpt(files, strength_to_step(1.0 if strength is None else strength, num_steps_eval), bool(sample_posterior))


def teacher_init_image_options(init_images, strength, sample_posterior, teacher_steps):
    """--network teacher with --init_images -> (files, entry step k of the --teacher_steps chain, sample the posterior?).  --strength
    has no natural default for the teacher (diffusers' 0.8 is not this tool's 1.0) and must be given."""
    if strength is None:
        raise click.UsageError(f'--init_images with --network {TEACHER}: image-to-image with the teacher sampler needs an explicit --strength '
                               '(the share of the --teacher_steps steps that run)')
    try:
        k = teacher_start_index(teacher_steps, strength)
    except ValueError as e:
        raise click.UsageError(f'--strength {strength:g} with --network {TEACHER}: {e}')
    return Img2ImgOpt(list_init_images(init_images), k, bool(sample_posterior))


def image_to_image_options(network_pkl, init_images, strength, sample_posterior, num_steps_eval, teacher_steps=None):
    """init_image_options for a snapshot (and for every refusal without --init_images), teacher_init_image_options for the teacher."""
    if network_pkl == TEACHER and init_images is not None:
        return teacher_init_image_options(init_images, strength, sample_posterior, TEACHER_STEPS if teacher_steps is None else teacher_steps)
    return init_image_options(network_pkl, init_images, strength, sample_posterior, num_steps_eval)


def list_mask_images(path, num_init):
    """The PNG / JPEG files of --mask_images, sorted by name: one for all samples, or one per init image."""
    return image_files(path, '--mask_images', expect=num_init)


def mask_options(init_images, mask_images, mask_composite, num_init):
    """-> None without --mask_images, else (mask files, composite the kept pixels?); the mask options need --init_images."""
    if mask_images is None:
        if mask_composite:
            raise click.UsageError('--mask_composite applies to --mask_images only')
        return None
    if init_images is None:
        raise click.UsageError('--mask_images applies to --init_images only: the init image is the region that is kept')
    return MaskOpt(list_mask_images(mask_images, num_init), bool(mask_composite))


def load_mask_image(path, resolution):
    """-> uint8 [resolution, resolution]: 'L', the centre crop of load_init_image, resized with PIL's NEAREST filter."""
    return _load_square(path, resolution, 'L', 'NEAREST')


def load_mask_batch(files, indices, resolution):
    """Sample idx takes file idx % len(files) -> uint8 [B, resolution, resolution]."""
    return _batch(load_mask_image, files, indices, resolution)


def latent_mask(pixel_mask):
    """uint8 [B, 8h, 8w] pixel masks -> uint8 [B, h, w]: 1 (repaint) where any pixel of the cell's 8 x 8 block is >= 128."""
    b, H, W = pixel_mask.shape
    return (pixel_mask.reshape(b, H // 8, 8, W // 8, 8) >= 128).any(axis=(2, 4)).astype(np.uint8)


def composite(generated, init_pixels, pixel_mask):
    """uint8 [B, H, W, 3] generated and init pixels, uint8 [B, H, W] masks -> the init pixels where the mask is < 128."""
    return np.where((pixel_mask >= 128)[..., None], generated, init_pixels)


def list_control_images(path):
    """The PNG / JPEG files of --control_images, sorted by name."""
    return image_files(path, '--control_images')


def control_options(controlnet, control_images, control_scale):
    """-> None without the ControlNet options, else (spec, control image files, scale); one of --controlnet / --control_images without
    the other, or --control_scale without them, is a usage error."""
    if controlnet is None and control_images is None:
        if control_scale is not None:
            raise click.UsageError('--control_scale applies to --controlnet / --control_images only')
        return None
    if controlnet is None:
        raise click.UsageError('--control_images needs --controlnet (a ControlNet directory or random:controlnet[:seed])')
    if control_images is None:
        raise click.UsageError('--controlnet needs --control_images (the directory of control images)')
    return ControlOpt(controlnet, list_control_images(control_images), 1.0 if control_scale is None else float(control_scale))


def load_control_image(path, resolution):
    """-> uint8 [resolution, resolution, 3] RGB.  The file must already have that size: nothing is cropped or resized."""
    import PIL.Image
    with PIL.Image.open(path) as im:
        w, h = im.size
        if (w, h) != (resolution, resolution):
            raise click.UsageError(f'--control_images: {path} is {w} x {h}, expected {resolution} x {resolution} (--resolution); '
                                   'control images are not resized')
        return np.ascontiguousarray(np.asarray(im.convert('RGB'), dtype=np.uint8))


def load_control_batch(files, indices, resolution):
    """Sample idx takes file idx % len(files) -> uint8 [B, resolution, resolution, 3]."""
    return _batch(load_control_image, files, indices, resolution)


def control_edge_options(controlnet, control_preprocess, canny_low, canny_high, control_adherence, edge_tolerance, resolution):
    """-> None without the edge options, else (make the hints with Canny?, low, high, score the adherence?, tolerance); every inconsistent
    option is refused by name, before a GPU is touched."""
    given = [f for f, v in (('--control_preprocess', control_preprocess), ('--canny_low', canny_low), ('--canny_high', canny_high),
                            ('--control_adherence', control_adherence or None), ('--edge_tolerance', edge_tolerance)) if v is not None]
    if not given:
        return None
    if controlnet is None:
        raise click.UsageError(f'{" / ".join(given)} apply to --controlnet only')
    if control_preprocess is None and not control_adherence:
        raise click.UsageError(f'{" / ".join(given)}: the Canny thresholds and the tolerance apply to --control_preprocess canny or --control_adherence 1')
    if edge_tolerance is not None and not control_adherence:
        raise click.UsageError('--edge_tolerance applies to --control_adherence 1 only')
    low, high = 100 if canny_low is None else canny_low, 200 if canny_high is None else canny_high
    tolerance = 1 if edge_tolerance is None else edge_tolerance
    for flag, v in (('--canny_low', low), ('--canny_high', high), ('--edge_tolerance', tolerance)):
        if v < 0:
            raise click.UsageError(f'{flag} {v}: cannot be negative')
    if low > high:
        raise click.UsageError(f'--canny_low {low} is above --canny_high {high}')
    if tolerance > edge_maps.MAX_TOLERANCE:
        raise click.UsageError(f'--edge_tolerance {tolerance}: at most {edge_maps.MAX_TOLERANCE} pixels')
    if edge_maps.hysteresis_lds_bytes(resolution, resolution) > edge_maps.HYST_LDS_MAX:
        raise click.UsageError(f'--resolution {resolution}: the Canny hysteresis keeps both bit planes of an image on chip, '
                               f'{edge_maps.hysteresis_lds_bytes(resolution, resolution)} bytes here against a limit of {edge_maps.HYST_LDS_MAX} (768 x 768)')
    return EdgeOpt(control_preprocess is not None, low, high, bool(control_adherence), tolerance)


def list_ip_images(path):
    """The PNG / JPEG files of --ip_images, sorted by name."""
    return image_files(path, '--ip_images')


def ip_options(ip_adapter, ip_image_encoder, ip_images, ip_scale):
    """-> None without the IP-Adapter options, else (adapter spec, image encoder spec, prompt image files, scale); one or two of
    --ip_adapter / --ip_image_encoder / --ip_images without the rest, or --ip_scale without them, is a usage error."""
    given = {'--ip_adapter': ip_adapter, '--ip_image_encoder': ip_image_encoder, '--ip_images': ip_images}
    if all(v is None for v in given.values()):
        if ip_scale is not None:
            raise click.UsageError('--ip_scale applies to --ip_adapter / --ip_image_encoder / --ip_images only')
        return None
    missing = [k for k, v in given.items() if v is None]
    if missing:
        have = [k for k, v in given.items() if v is not None]
        raise click.UsageError(f'{" / ".join(have)} need{"s" if len(have) == 1 else ""} {" and ".join(missing)} (an IP-Adapter file or '
                               'random:ip-adapter[:seed], a CLIP image encoder directory or random:clip-<arch>, and the directory of prompt images)')
    return IpOpt(ip_adapter, ip_image_encoder, list_ip_images(ip_images), 1.0 if ip_scale is None else float(ip_scale))


def lora_options(lora, lora_scale):
    """-> None without --lora, else (specs, scales): --lora_scale may be given never, once (for all files) or once per file; anything
    else, and --lora_scale without --lora, is a usage error."""
    try:
        scales = lora_scales(len(lora or ()), lora_scale)
    except ValueError as e:
        raise click.UsageError(str(e))
    return LoraOpt(list(lora), scales) if lora else None


def fidelity_options(init_images, fidelity, lpips_vgg, lpips_lin, diversity=False):
    """-> None without --fidelity, else (lpips_vgg, lpips_lin) (both None: PSNR and SSIM only); inconsistent options are refused."""
    given = [f for f, v in (('--lpips_vgg', lpips_vgg), ('--lpips_lin', lpips_lin)) if v is not None]
    if not fidelity:
        if given and not diversity:
            raise click.UsageError(f'{" / ".join(given)} apply to --fidelity or --diversity only')
        return None
    if init_images is None:
        raise click.UsageError('--fidelity applies to --init_images only: an output is compared with the init image it started from')
    if given:
        try:
            check_lpips_specs(lpips_vgg, lpips_lin)
        except ValueError as e:
            raise click.UsageError(str(e))
    return FidelityOpt(lpips_vgg, lpips_lin)


def diversity_options(diversity, seeds_per_prompt, lpips_vgg, lpips_lin, keys):
    """-> None without --diversity, else (lpips_vgg, lpips_lin, {group: [sample keys]}); `keys` are the samples' indices (the index
    that picks a sample's condition).  Inconsistent options are refused by name."""
    if not diversity:
        return None
    if seeds_per_prompt < 2:
        raise click.UsageError('--diversity needs --seeds_per_prompt K with K >= 2: the K samples of one prompt are compared with each other')
    try:
        prompt_diversity.check_group_size(seeds_per_prompt)
        check_lpips_specs(lpips_vgg, lpips_lin)
    except ValueError as e:
        raise click.UsageError(f'--diversity: {e}')
    if len(keys) % seeds_per_prompt:
        raise click.UsageError(f'--diversity: {len(keys)} samples (--seeds, --num) are not a multiple of --seeds_per_prompt {seeds_per_prompt}')
    try:
        return DiversityOpt(lpips_vgg, lpips_lin, prompt_diversity.groups_of(keys, seeds_per_prompt))
    except ValueError as e:
        raise click.UsageError(f'--diversity: {e}')


def sample_path(outdir, subdirs, key):
    """Where sample `key` is written."""
    return os.path.join(os.path.join(outdir, f'{key - key % 1000:06d}') if subdirs else outdir, f'{key:06d}.png')


def load_png_group(paths, device):
    """The written files of one group, read back (PNG is lossless: these are the bits that were written) -> uint8 [K, 3, H, W]."""
    import PIL.Image
    arrs = []
    for path in paths:
        with PIL.Image.open(path) as im:
            arrs.append(np.asarray(im.convert('RGB'), dtype=np.uint8))
    return torch.from_numpy(np.stack(arrs)).to(device).permute(0, 3, 1, 2).contiguous()


def load_ip_image(path):
    """-> uint8 [3, H, W] RGB, any size: the image encoder's transform resizes."""
    import PIL.Image
    with PIL.Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'), dtype=np.uint8).transpose(2, 0, 1))


def ip_image_embeds(files, indices, tower, device):
    """Sample idx takes file idx % len(files) -> image embeddings [B, E] fp32; one tower call per image (the files may differ in size)."""
    with torch.no_grad():
        return torch.cat([tower(torch.from_numpy(load_ip_image(files[i % len(files)])).to(device)[None]).float() for i in indices])


def write_report(rows, path, options, rows_key, aggregate, sort_key=None):
    """This rank's `rows` merged with every other rank's and sorted by key (`sort_key`: the order of the keys, which are written as
    strings) -> dict(options=, <rows_key>=, mean=aggregate(rows)) on every rank; rank 0 writes it to `path` with indent 1 (inf / nan
    as Infinity / NaN, which json.load reads back), in a directory made if need be."""
    if dist.get_world_size() > 1:
        parts = [None] * dist.get_world_size()
        torch.distributed.all_gather_object(parts, rows)
        rows = {k: v for part in parts for k, v in part.items()}
    rows = {str(k): rows[k] for k in sorted(rows, key=sort_key)}
    report = {'options': options, rows_key: rows, 'mean': aggregate(rows)}
    if dist.get_rank() == 0:
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        with open(path, 'w') as f:
            json.dump(report, f, indent=1)
    return report


Networks = NamedTuple('Networks', [('G_ema', object), ('vae', object), ('sched', object), ('text_encoder', object), ('tokenizer', object)])


def load_generator(network_pkl, repo_id, device, text_encoder_kind, teacher, solver_kw=None):
    """-> Networks(G_ema, vae, sched, text_encoder, tokenizer) of --repo_id; G_ema is the 'ema' of the snapshot pickle, or with `teacher`
    (a TeacherOpt; `solver_kw`: teacher_solver_options') the UNet of --repo_id itself."""
    if teacher is None:
        dist.print0(f'Loading network from "{network_pkl}"...')
        with open(network_pkl, 'rb') as f:
            G_ema = pickle.load(f)['ema'].to(device)
    elif solver_kw is None:
        dist.print0(f'Sampling the teacher "{repo_id}": DDIM {teacher.steps} steps, guidance scale {teacher.guidance_scale:g}')
    else:
        dist.print0(f'Sampling the teacher "{repo_id}": {solver_kw["solver"]} {teacher.steps} steps, spacing {solver_kw["spacing"] or "of the model"}, '
                    f'eta {solver_kw["eta"]:g}, guidance scale {teacher.guidance_scale:g}, rescale {solver_kw["guidance_rescale"]:g}')
    unet, vae, sched, text_encoder, tokenizer = load_sd15(repo_id, repo_id, device, torch.bfloat16, text_encoder=text_encoder_kind)
    if teacher is None:
        del unet
        check_prediction_type(G_ema, sched)       # a v snapshot with an epsilon --repo_id (or the reverse) would sample garbage
    else:
        G_ema = unet
    G_ema.eval().requires_grad_(False)
    return Networks(G_ema, vae, sched, text_encoder, tokenizer)


def sample_images(net, z, prompts, resolution, teacher, solver_kw=None, init_timestep=None, num_steps_eval=1, randn=None, **conditions):
    """The decoded images fp32 NCHW of latents z under `prompts`: the snapshot's sampler, or with `teacher` the DDIM loop, or with `solver_kw`
    too the solver family (`randn`: its per-step noise).  `conditions`: the samplers' keywords, as build_conditions makes them."""
    common = dict(unet=net.G_ema, latents=z, contexts=prompts, noise_scheduler=net.sched, text_encoder=net.text_encoder, tokenizer=net.tokenizer,
                  resolution=resolution, return_images=True, vae=net.vae, **conditions)
    with torch.no_grad():
        if teacher is None:
            return sid_sd_sampler(init_timesteps=init_timestep * torch.ones(len(z), device=z.device, dtype=torch.long), dtype=torch.bfloat16,
                                  num_steps=1, train_sampler=False, num_steps_eval=num_steps_eval, **common)
        common.update(guidance_scale=teacher.guidance_scale, num_inference_steps=teacher.steps)
        if solver_kw is None:
            return teacher_sample_i2i(**common)
        kw = {k: v for k, v in solver_kw.items() if k != 'negative_prompt'}
        neg = None if solver_kw['negative_prompt'] is None else [solver_kw['negative_prompt']] * len(z)
        return teacher_sample_solver_i2i(negative_contexts=neg, randn=randn, **kw, **common)


def to_uint8_nhwc(images):
    """Images fp32 NCHW in [-1, 1] -> the uint8 [B, H, W, 3] array that is written: (img * 127.5 + 128).clip(0, 255)."""
    return (images.float() * 127.5 + 128).clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


def load_models(o, network_pkl, repo_id, device, text_encoder_kind, num_steps_eval):
    """What the resolved options `o` need, loaded once -> one namespace: net (load_generator's Networks, the LoRA files merged), and
    vae_encoder, control_net, ip_tower, ip_net, lpips, each None where its option is absent."""
    net = load_generator(network_pkl, repo_id, device, text_encoder_kind, o.teacher, o.solver)
    m = SimpleNamespace(net=net, vae_encoder=None, control_net=None, ip_tower=None, ip_net=None, lpips=None)
    if o.teacher is not None and num_steps_eval != 1:
        dist.print0(f'Note: --num_steps_eval {num_steps_eval} is ignored with --network {TEACHER} (the step count is --teacher_steps)')
    if o.lora is not None:           # merged once, before anything derives from the weights; the sampling loop does not change
        load_lora(o.lora.specs, o.lora.scales, net.G_ema, net.text_encoder, log=dist.print0)
    if o.img2img is not None:
        m.vae_encoder = load_vae_encoder(repo_id, device)
        dist.print0(f'Image-to-image: {len(o.img2img.files)} init images from "{o.dirs.init}", entering at step {o.img2img.start} of '
                    f'{num_steps_eval if o.teacher is None else o.teacher.steps}')
    if o.control is not None:
        m.control_net = load_controlnet(o.control.spec, net.G_ema, device)
        dist.print0(f'ControlNet "{o.control.spec}": scale {o.control.scale:g}, {len(o.control.files)} control image(s) from "{o.dirs.control}"')
        if o.edge is not None:
            dist.print0(f'Canny {o.edge.low} / {o.edge.high}:' + (' control images made from the files of --control_images;' if o.edge.preprocess else '')
                        + (f' edge adherence with a tolerance of {o.edge.tolerance} pixel(s)' if o.edge.adherence else ''))
    if o.ip is not None:
        m.ip_tower = load_clip_vision(o.ip.image_encoder, device, net.G_ema.compute_dtype)
        m.ip_net = load_ip_adapter(o.ip.adapter, net.G_ema, device, m.ip_tower.cfg.projection_dim)
        dist.print0(f'IP-Adapter "{o.ip.adapter}": {m.ip_net.tokens} image tokens, scale {o.ip.scale:g}, image encoder "{o.ip.image_encoder}", '
                    f'{len(o.ip.files)} prompt image(s) from "{o.dirs.ip}"')
    if o.masks is not None:
        dist.print0(f'Inpainting: {len(o.masks.files)} mask image(s) from "{o.dirs.mask}"' + (', kept pixels composited from the init images' if o.masks.composite else ''))
    if o.fid is not None:
        m.lpips = load_lpips(o.fid.lpips_vgg, o.fid.lpips_lin, device) if o.fid.lpips_vgg is not None else None
        dist.print0('Fidelity against the init images: PSNR, SSIM' + (f', LPIPS-VGG "{o.fid.lpips_vgg}" / "{o.fid.lpips_lin}"' if m.lpips is not None else ''))
    return m


def build_conditions(o, m, rnd, cond, resolution, device):
    """The conditioning of one batch, `cond` the index that selects each sample's files -> (the samplers' keywords init_latents, start_step or
    start_index, mask, control, ip; the sources kept for compositing and scoring).  The posterior's eps is the second draw from `rnd`, after z."""
    i2i, src = {}, SimpleNamespace(init_pixels=None, pixels=None, pixel_mask=None, control_edges=None)
    dup = 2 if (o.teacher is not None and o.teacher.guidance_scale != 1) else 1          # the guided teacher batch is [uncond ; cond]
    if o.img2img is not None:
        src.init_pixels = load_init_batch(o.img2img.files, cond, resolution)
        src.pixels = torch.from_numpy(src.init_pixels).to(device)
        eps = rnd.randn([len(cond), 4, resolution // 8, resolution // 8], device=device) if o.img2img.sample_posterior else None
        i2i = {'init_latents': m.vae_encoder.encode_latents(src.pixels, eps=eps), 'start_step' if o.teacher is None else 'start_index': o.img2img.start}
        if o.masks is not None:
            src.pixel_mask = load_mask_batch(o.masks.files, cond, resolution)
            i2i['mask'] = torch.from_numpy(latent_mask(src.pixel_mask)).to(device)
    if o.control is not None:        # one conversion launch + the hint embedder, once per batch
        if o.edge is not None and o.edge.preprocess:      # photographs: the crop of load_init_image, then their Canny map, made on the device
            src.control_edges = edge_maps.canny(torch.from_numpy(load_init_batch(o.control.files, cond, resolution)).to(device), o.edge.low, o.edge.high, rgb=True)
            hints = src.control_edges.rgb_u8()
        else:
            hints = torch.from_numpy(load_control_batch(o.control.files, cond, resolution)).to(device)
            if o.edge is not None:
                src.control_edges = edge_maps.pack(hints)
        i2i['control'] = m.control_net.prepare(hints, scale=o.control.scale, dup=dup)
    if o.ip is not None:             # the image tower, the projection and ONE k|v GEMM for all layers, once per batch
        i2i['ip'] = m.ip_net.prepare(ip_image_embeds(o.ip.files, cond, m.ip_tower, device), scale=o.ip.scale, dup=dup)
    return i2i, src


def score_written(o, m, src, arr, names, device, fid_rows, adh_rows):
    """`arr`, the uint8 that goes into the PNG files `names`, scored on the device: against the crop load_init_image produced (--fidelity
    -> fid_rows) and its Canny edges against the control image's edge set (--control_adherence -> adh_rows)."""
    if o.fid is not None:
        rows = score_batch(src.pixels.permute(0, 3, 1, 2).contiguous(), torch.from_numpy(np.ascontiguousarray(arr)).to(device).permute(0, 3, 1, 2).contiguous(),
                           None if o.masks is None else torch.from_numpy(src.pixel_mask).to(device), m.lpips)
        fid_rows.update(zip(names, rows))
    if o.edge is not None and o.edge.adherence:
        rows = edge_maps.score_batch(src.control_edges, torch.from_numpy(np.ascontiguousarray(arr)).to(device), o.edge.low, o.edge.high, o.edge.tolerance)
        adh_rows.update(zip(names, rows))


@click.command()
@click.option('--network', 'network_pkl', type=str, required=True, metavar='PATH', help=f'Network snapshot pickle, or "{TEACHER}": sample the UNet of --repo_id itself')
@click.option('--outdir', type=str, required=True, metavar='DIR', help='Where to save the output images')
@click.option('--seeds', type=parse_int_list, default='0-63', show_default=True, metavar='LIST', help='Random seeds (e.g. 1,2,5-10)')
@click.option('--subdirs', is_flag=True, help='Create subdirectory for every 1000 seeds')
@click.option('--batch', 'max_batch_size', type=click.IntRange(min=1), default=16, show_default=True, help='Maximum batch size')
@click.option('--num', 'num_fid_samples', type=click.IntRange(min=1), default=30000, show_default=True, help='Maximum number of images')
@click.option('--init_timestep', type=click.IntRange(min=0), default=625, show_default=True, help='t_init, in [0,999]')
@click.option('--text_prompts', type=str, default='prompts/captions.txt', show_default=True, help='Prompt file, one per line')
@click.option('--repo_id', type=str, default='runwayml/stable-diffusion-v1-5', show_default=True, help='Local diffusers directory, random:<arch> or random:<arch>:v')
@click.option('--resolution', type=click.IntRange(min=8), default=512, show_default=True, help='Image resolution (latent = resolution / 8)')
@click.option('--use_fp16', type=bool, default=True, show_default=True, help='Accepted for compatibility (compute is bf16)')
@click.option('--enable_compress_npz', type=bool, default=False, show_default=True, help='Also write the batch as images.npz')
@click.option('--num_steps_eval', type=click.IntRange(min=0), default=1, show_default=True, help='Generation steps (1 = one-step)')
@click.option('--custom_seed', type=bool, default=False, show_default=True, help='Prompt i <-> i-th seed of the list instead of seed value')
@click.option('--teacher_steps', type=click.IntRange(min=1), default=None, help=f'DDIM steps of --network {TEACHER}  [default: {TEACHER_STEPS}]')
@click.option('--guidance_scale', type=float, default=None, help=f'Classifier-free guidance scale of --network {TEACHER}  [default: {TEACHER_CFG}]')
@click.option('--teacher_sampler', type=click.Choice(['ddim', 'dpmpp2m']), default=None, help=f'Solver of --network {TEACHER}: DDIM or DPM-Solver++ 2M  [default: ddim]')
@click.option('--teacher_spacing', type=click.Choice(['leading', 'trailing', 'linspace']), default=None, help=f'Timestep spacing of --network {TEACHER}  [default: the timestep_spacing of --repo_id]')
@click.option('--teacher_eta', type=click.FloatRange(min=0), default=None, help='DDIM eta: 0 deterministic, 1 ancestral; noise from the per-seed generator, after z  [default: 0]')
@click.option('--guidance_rescale', type=click.FloatRange(min=0, max=1), default=None, help=f'Guidance rescale phi (Lin et al. 2024) of --network {TEACHER}  [default: 0]')
@click.option('--negative_prompt', type=str, default=None, help=f"Prompt of the unconditional half of --network {TEACHER}  [default: '']")
@click.option('--init_images', type=str, default=None, metavar='DIR', help='Image-to-image: PNG/JPEG files (sorted by name); sample idx starts from file idx mod len(files)')
@click.option('--strength', type=click.FloatRange(min=0, max=1, min_open=True), default=None,
              help='With --init_images: share of the --num_steps_eval steps that run, k = N - ceil(S N) is the entry step; a one-step '
                   'generator has no such choice, its knob is --init_timestep  [default: 1]')
@click.option('--sample_posterior', type=bool, default=None, help='With --init_images: sample the VAE posterior (eps from the per-seed generator, after z) instead of its mean  [default: False]')
@click.option('--mask_images', type=str, default=None, metavar='DIR', help='Inpainting, with --init_images: mask files (sorted by name; one for all, or one per init image), >= 128 = repaint')
@click.option('--mask_composite', type=bool, default=False, show_default=True, help='With --mask_images: take the pixels whose mask value is < 128 from the init image after decoding')
@click.option('--controlnet', type=str, default=None, metavar='SPEC', help='ControlNet: a local diffusers-layout directory, or random:controlnet[:seed]; needs --control_images')
@click.option('--control_images', type=str, default=None, metavar='DIR', help='Control images, already --resolution square: PNG/JPEG files (sorted by name); sample idx uses file idx mod len(files)')
@click.option('--control_scale', type=click.FloatRange(min=0), default=None, help='Scale of the ControlNet residuals  [default: 1]')
@click.option('--control_preprocess', type=click.Choice(['canny']), default=None, help='--control_images holds photographs of any size: centre crop, LANCZOS resize, and their Canny edge map (made on the device) is the control image')
@click.option('--canny_low', type=int, default=None, help='Lower Canny threshold of --control_preprocess / --control_adherence  [default: 100]')
@click.option('--canny_high', type=int, default=None, help='Upper Canny threshold of --control_preprocess / --control_adherence  [default: 200]')
@click.option('--control_adherence', type=bool, default=False, show_default=True, help='With --controlnet: precision / recall / F1 of the Canny edges of every written image against the edges of its control image -> <outdir>/control_adherence.json')
@click.option('--edge_tolerance', type=int, default=None, help='With --control_adherence: an edge pixel is a hit within this many pixels (Chebyshev) of an edge of the other set  [default: 1]')
@click.option('--ip_adapter', type=str, default=None, metavar='SPEC', help='IP-Adapter (image prompt): a local .safetensors / .bin file, or random:ip-adapter[:seed]; needs --ip_image_encoder and --ip_images')
@click.option('--ip_image_encoder', type=str, default=None, metavar='DIR', help='CLIP image encoder of --ip_adapter: a local directory (config.json, model.safetensors), or random:clip-<arch>')
@click.option('--ip_images', type=str, default=None, metavar='DIR', help='Prompt images of --ip_adapter, any size: PNG/JPEG files (sorted by name); sample idx uses file idx mod len(files)')
@click.option('--ip_scale', type=click.FloatRange(min=0), default=None, help='Scale of the image attention  [default: 1]')
@click.option('--lora', type=str, multiple=True, metavar='SPEC', help='LoRA file merged into the UNet and the text encoder (repeatable): a local kohya / diffusers .safetensors / .bin / .pt file, or random:lora[:rank[:seed]]')
@click.option('--lora_scale', type=float, multiple=True, help='Scale of --lora (repeatable: one for all files, or one per file; negative allowed)  [default: 1]')
@click.option('--fidelity', type=bool, default=False, show_default=True, help='With --init_images: PSNR / SSIM (and LPIPS) of every written image against its init image -> <outdir>/fidelity.json')
@click.option('--lpips_vgg', type=str, default=None, metavar='SPEC', help='With --fidelity: a torch.save\'d torchvision VGG16 state dict, or random:lpips-vgg[:seed]; needs --lpips_lin')
@click.option('--lpips_lin', type=str, default=None, metavar='SPEC', help='With --fidelity: the lin weights of the lpips package (its vgg.pth), or random:lpips-vgg[:seed]; needs --lpips_vgg')
@click.option('--seeds_per_prompt', type=click.IntRange(min=1), default=1, show_default=True, help='K samples per condition: sample idx keeps its seed and file name and takes prompt (and init / mask / control / IP image) idx // K')
@click.option('--diversity', type=bool, default=False, show_default=True, help='With --seeds_per_prompt K >= 2 and --lpips_vgg / --lpips_lin: all-pairs LPIPS (and SSIM, MSE) among the K samples of every prompt -> <outdir>/diversity.json')
@click.option('--text_encoder', type=click.Choice(['torch', 'hip']), default=None, help='CLIP text encoder: the PyTorch module, or the same weights on the HIP kernels  [default: $SIDLSG_TEXT_ENCODER, else torch] (not a reference option)')
def main(network_pkl, outdir, seeds, subdirs, max_batch_size, num_fid_samples, init_timestep, text_prompts, repo_id, resolution, use_fp16,
         enable_compress_npz, num_steps_eval, custom_seed, teacher_steps, guidance_scale, init_images, strength, sample_posterior, text_encoder,
         teacher_sampler, teacher_spacing, teacher_eta, guidance_rescale, negative_prompt, mask_images, mask_composite, controlnet, control_images,
         control_scale, ip_adapter, ip_image_encoder, ip_images, ip_scale, fidelity, lpips_vgg, lpips_lin, lora, lora_scale, seeds_per_prompt, diversity,
         control_preprocess, canny_low, canny_high, control_adherence, edge_tolerance):
    if resolution % 8:
        raise click.BadParameter(f'{resolution}: must be a multiple of 8', param_hint='--resolution')
    seeds = seeds[:num_fid_samples]
    # the options, resolved: every usage error comes from these lines, in this order, before a GPU is touched (dirs: as given, for the messages)
    o = SimpleNamespace(dirs=SimpleNamespace(init=init_images, mask=mask_images, control=control_images, ip=ip_images))
    o.teacher = teacher_options(network_pkl, teacher_steps, guidance_scale)
    o.solver = teacher_solver_options(network_pkl, teacher_sampler, teacher_spacing, teacher_eta, guidance_rescale, negative_prompt)
    o.img2img = image_to_image_options(network_pkl, init_images, strength, sample_posterior, num_steps_eval, teacher_steps)
    o.masks = mask_options(init_images, mask_images, mask_composite, 0 if o.img2img is None else len(o.img2img.files))
    o.control = control_options(controlnet, control_images, control_scale)
    o.edge = control_edge_options(controlnet, control_preprocess, canny_low, canny_high, control_adherence, edge_tolerance, resolution)
    o.ip = ip_options(ip_adapter, ip_image_encoder, ip_images, ip_scale)
    o.fid = fidelity_options(init_images, fidelity, lpips_vgg, lpips_lin, diversity)
    o.lora = lora_options(lora, lora_scale)
    o.div = diversity_options(diversity, seeds_per_prompt, lpips_vgg, lpips_lin, list(range(len(seeds))) if custom_seed else [int(s) for s in seeds])
    dist.init()
    device = torch.device('cuda')
    rank, world = dist.get_rank(), dist.get_world_size()
    captions = read_prompts(text_prompts)
    num_batches = ((len(seeds) - 1) // (max_batch_size * world) + 1) * world
    index = torch.arange(len(seeds)) if custom_seed else torch.as_tensor(seeds)
    rank_batches = index.tensor_split(num_batches)[rank::world]

    if world > 1 and rank != 0:
        torch.distributed.barrier()                    # rank 0 touches the files first
    m = load_models(o, network_pkl, repo_id, device, text_encoder, num_steps_eval)
    if world > 1 and rank == 0:
        torch.distributed.barrier()
    if o.teacher is None and num_steps_eval > 1:
        outdir = f'{outdir}_numstep{num_steps_eval}'

    fid_rows, adh_rows = {}, {}
    dist.print0(f'Generating {len(seeds)} images to "{outdir}"...')
    for batch in rank_batches:
        if world > 1:
            torch.distributed.barrier()
        if len(batch) == 0:
            continue
        batch = [int(b) for b in batch]
        rnd = StackedRandomGenerator(device, [seeds[i] for i in batch] if custom_seed else batch)
        z = rnd.randn([len(batch), 4, resolution // 8, resolution // 8], device=device)
        cond = [i // seeds_per_prompt for i in batch]          # the index that selects a sample's condition; K = 1: the sample's own
        i2i, src = build_conditions(o, m, rnd, cond, resolution, device)
        images = sample_images(m.net, z, [captions[i % len(captions)] for i in cond], resolution, o.teacher, o.solver, init_timestep, num_steps_eval,
                               randn=lambda shape: rnd.randn(list(shape), device=device), **i2i)
        arr = to_uint8_nhwc(images)
        if o.masks is not None and o.masks.composite:
            arr = composite(arr, src.init_pixels, src.pixel_mask)
        score_written(o, m, src, arr, [f'{key:06d}.png' for key in batch], device, fid_rows, adh_rows)
        for key, img in zip(batch, arr):
            path = sample_path(outdir, subdirs, key)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            save_png(path, np.ascontiguousarray(img))
        if enable_compress_npz:
            np.savez_compressed(os.path.join(outdir, f'images_{batch[0]:06d}.npz'), images=arr)
    if o.fid is not None:
        report = write_report(fid_rows, os.path.join(outdir, 'fidelity.json'),
                              dict(network=network_pkl, init_images=init_images, mask_images=mask_images, mask_composite=bool(mask_composite),
                                   strength=strength, init_timestep=init_timestep, num_steps_eval=num_steps_eval, resolution=resolution,
                                   teacher_steps=teacher_steps, controlnet=controlnet, ip_adapter=ip_adapter, lpips_vgg=o.fid.lpips_vgg,
                                   lpips_lin=o.fid.lpips_lin), 'per_image', aggregate_fidelity)
        dist.print0(f'Fidelity over {len(report["per_image"])} images: {format_means(report["mean"])}')
    if o.edge is not None and o.edge.adherence:
        report = write_report(adh_rows, os.path.join(outdir, 'control_adherence.json'),
                              dict(network=network_pkl, controlnet=controlnet, control_images=control_images, control_preprocess=control_preprocess,
                                   control_scale=o.control.scale, canny_low=o.edge.low, canny_high=o.edge.high, edge_tolerance=o.edge.tolerance,
                                   resolution=resolution, init_timestep=init_timestep, num_steps_eval=num_steps_eval, teacher_steps=teacher_steps,
                                   init_images=init_images, mask_images=mask_images, mask_composite=bool(mask_composite), ip_adapter=ip_adapter),
                              'per_image', edge_maps.aggregate)
        dist.print0(f'Control adherence over {edge_maps.format_means(report["mean"])}')
    if o.div is not None:            # after every file is written: group g is scored by rank g mod world from the files read back
        if world > 1:
            torch.distributed.barrier()
        lpips_div, div_rows = load_lpips(o.div.lpips_vgg, o.div.lpips_lin, device), {}
        for n, (g, keys) in enumerate(o.div.groups.items()):
            if n % world == rank:
                row = prompt_diversity.score_groups(load_png_group([sample_path(outdir, subdirs, k) for k in keys], device), seeds_per_prompt, lpips_div)[0]
                div_rows[g] = dict(prompt=captions[g % len(captions)], files=[f'{k:06d}.png' for k in keys], **row)
        report = write_report(div_rows, os.path.join(outdir, 'diversity.json'),
                              dict(network=network_pkl, seeds_per_prompt=seeds_per_prompt, text_prompts=text_prompts, resolution=resolution,
                                   init_timestep=init_timestep, num_steps_eval=num_steps_eval, teacher_steps=teacher_steps,
                                   guidance_scale=guidance_scale, init_images=init_images, controlnet=controlnet, ip_adapter=ip_adapter,
                                   lpips_vgg=o.div.lpips_vgg, lpips_lin=o.div.lpips_lin), 'per_prompt', prompt_diversity.aggregate)
        dist.print0(f'Diversity over {prompt_diversity.format_means(report["mean"])}')
    if world > 1:
        torch.distributed.barrier()
    dist.print0('Done.')


if __name__ == '__main__':
    main()
