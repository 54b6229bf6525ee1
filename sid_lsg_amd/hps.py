"""HPSv2 benchmark score from a local checkpoint (the fourth number the reference reports).

Reference: generate_hpsv2.py (the generation loop: for each of the four styles of `hpsv2.benchmark_prompts('all')`, image `seed` is
generated from prompt `seed` of that style and the latent of torch.Generator(seed), written as `<outdir>/<style>/<seed:05d>.jpg`;
then `hpsv2.evaluate(outdir)`) and the hpsv2 package's published source (`img_score.py`: open_clip ViT-H/14 with the fine-tuned
HPS_v2_compressed.pt, `preprocess_val` on the JPEG read back, score = the diagonal of image_features @ text_features.T of the
normalised features, no logit scale; `evaluate_benchmark`: per style the mean and the standard deviation of the means of groups
of 80, and the average over every image, all times 100).

Neither the package nor open_clip is needed here: the scorer is `clip.load_open_clip(checkpoint, tokenizer_dir)` -- the ViT on the
HIP kernels behind open_clip's validation transform in one launch (ops.pil_patches, bit-equal to Pillow + ToTensor + Normalize) --
and the benchmark prompts are read from a local directory in the package's layout.  The aggregation restates the package's
`evaluate_benchmark` from its published source; the package is absent offline, so that restatement is not pinned against it.
"""
import io
import json
import os

import numpy as np
import torch

STYLES = ('anime', 'concept-art', 'paintings', 'photo')
GROUP = 80                  # evaluate_benchmark: the spread is taken over the means of consecutive groups of 80 images
PROMPTS_PER_STYLE = 800
RESULT_FILE = 'hpsv2.json'


def benchmark_prompts(path):
    """{style: [prompt, ...]} from `<path>/<style>.json` for the four styles (each a JSON list of strings: the layout of the hpsv2
    package's benchmark directory).  Refuses, naming the file, when one is missing or is not such a list."""
    if not path or not os.path.isdir(str(path)):
        raise FileNotFoundError(f'HPSv2 benchmark prompts: {path!r} is not a directory (expected {", ".join(s + ".json" for s in STYLES)} in it)')
    out = {}
    for style in STYLES:
        f = os.path.join(str(path), style + '.json')
        if not os.path.isfile(f):
            raise FileNotFoundError(f'HPSv2 benchmark prompts: {f} is missing')
        with open(f) as fh:
            prompts = json.load(fh)
        if not isinstance(prompts, list) or not prompts or not all(isinstance(p, str) for p in prompts):
            raise ValueError(f'HPSv2 benchmark prompts: {f} is not a non-empty JSON list of strings')
        out[style] = prompts
    return out


def score(detector, images_u8, prompts):
    """[B] fp32 HPS of image i under prompt i: the cosine of the normalised image and text embeddings (no logit scale).
    detector: clip.HipCLIPDetector (load_open_clip); images_u8: uint8 [B, 3, H, W] on its device."""
    if len(prompts) != len(images_u8):
        raise ValueError(f'hps.score: {len(images_u8)} images and {len(prompts)} prompts')
    return detector.scores(images_u8, list(prompts))


def aggregate(scores_by_style):
    """{style: [score, ...]} -> {style: 100 x mean, style + '_std': 100 x the standard deviation (population) of the means of
    consecutive groups of 80, 'Average': 100 x the mean over all images}, the numbers `evaluate_benchmark` prints."""
    out, everything = {}, []
    for style, s in scores_by_style.items():
        s = np.asarray([float(v) for v in s], dtype=np.float64)
        if s.size == 0:
            raise ValueError(f'hps.aggregate: no scores for style {style!r}')
        groups = [s[i:i + GROUP].mean() for i in range(0, s.size, GROUP)]
        out[style] = float(s.mean() * 100)
        out[style + '_std'] = float(np.std(groups) * 100)
        everything.append(s)
    out['Average'] = float(np.concatenate(everything).mean() * 100)
    return out


def format_table(result):
    """The lines evaluate_benchmark prints: style, score, spread."""
    lines = [f'{s:<15}{result[s]:.2f}\t{result[s + "_std"]:.4f}' for s in STYLES if s in result]
    return '\n'.join(lines + [f'{"Average":<15}{result["Average"]:.2f}'])


def jpeg_bytes(image_hwc_u8):
    """uint8 [H, W, 3] -> the JPEG PIL writes with its default quality (what generate_hpsv2.py's `.save(path)` leaves)."""
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(np.ascontiguousarray(image_hwc_u8), 'RGB').save(buf, format='JPEG')
    return buf.getvalue()


def read_image(src):
    """A file path or encoded bytes -> uint8 [3, H, W] RGB tensor (how the scorer opens an image)."""
    import PIL.Image
    with PIL.Image.open(io.BytesIO(src) if isinstance(src, (bytes, bytearray)) else src) as im:
        return torch.from_numpy(np.array(im.convert('RGB'), dtype=np.uint8)).permute(2, 0, 1).contiguous()


def jpeg_round_trip(images_u8):
    """uint8 [B, 3, H, W] (any device) -> the same batch after PIL's JPEG encoder and decoder, on the same device."""
    hwc = images_u8.permute(0, 2, 3, 1).cpu().numpy()
    return torch.stack([read_image(jpeg_bytes(i)) for i in hwc]).to(images_u8.device)


def image_path(outdir, style, seed, subdirs=False):
    d = os.path.join(outdir, style, f'{seed - seed % 1000:06d}') if subdirs else os.path.join(outdir, style)
    return os.path.join(d, f'{seed:05d}.jpg')


def score_directory(detector, outdir, prompts, seeds, subdirs=False, batch=16, rank=0, world=1):
    """{style: [score of seeds[0], ...]} for this rank's share (seeds[rank::world]) of the JPEG files of `outdir`, read back as the
    scorer sees them.  A missing file is an error."""
    out = {}
    mine = list(seeds)[rank::world]
    for style in STYLES:
        vals = []
        for i in range(0, len(mine), batch):
            chunk = mine[i:i + batch]
            files = [image_path(outdir, style, s, subdirs) for s in chunk]
            for f in files:
                if not os.path.isfile(f):
                    raise FileNotFoundError(f'HPSv2: {f} is missing')
            images = [read_image(f) for f in files]
            texts = [prompts[style][s] for s in chunk]
            if len({tuple(t.shape) for t in images}) == 1:
                vals += score(detector, torch.stack(images).to(detector.device), texts).cpu().tolist()
            else:                                      # files of different sizes (a directory somebody else wrote): one at a time
                for t, p in zip(images, texts):
                    vals += score(detector, t[None].to(detector.device), [p]).cpu().tolist()
        out[style] = vals
    return out


def gather_scores(scores_by_style, seeds, rank, world, device):
    """Every rank's score_directory share -> the full lists in seed-list order on every rank (one all_reduce per style)."""
    if world == 1:
        return scores_by_style
    out = {}
    for style in STYLES:
        full = torch.zeros(len(seeds), dtype=torch.float64, device=device)
        full[rank::world] = torch.tensor(scores_by_style[style], dtype=torch.float64, device=device)
        torch.distributed.all_reduce(full)
        out[style] = full.cpu().tolist()
    return out
