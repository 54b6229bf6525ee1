"""Evaluation metrics of the distilled generator: FID, CLIP scores, precision / recall, HPSv2, KID, CMMD and the Inception Score.

Reference: metrics/sid_metric_main.py:25-123 (registry, `calc_metric`, `report_metric`, the `fid30k_full` /
`fid_clip_30k_full` / `fid_test` / `fid_clip_test` entries), metrics/sid_fid_and_clip.py:32-74 (the Frechet distance between
the Inception feature statistics of generated images and of the real set), metrics/sid_metric_utils.py:112-188
(`FeatureStats`) and :412-510 (the generation loop: prompts through the InfiniteSampler, z ~ N(0, I) at resolution / 8,
uint8 images, 256 x 256 PIL-LANCZOS resize for the detector (reproduced bit for bit on the GPU); the CLIP score is the mean cosine of the detector's image | text halves;
a CLIP directory in the Hugging Face layout is scored by sid_lsg_amd.clip: the ViT image tower on the HIP kernels).

What is different here (not a translation):
  * the feature statistics live ON THE GPU in fp64 (`FeatureStats.raw_mean / raw_cov` are device tensors; x^T x is one
    fp64 GEMM per batch) and ranks are merged with ONE all_reduce of (sum, sum of outer products, count) at the end instead
    of a broadcast of every feature batch from every rank;
  * trace(sqrtm(S_g S_r)) is evaluated as the sum of the square roots of the eigenvalues of the symmetric PSD matrix
    S_r^1/2 S_g S_r^1/2 (two `torch.linalg.eigh` in fp64) -- no general matrix square root, no complex arithmetic; equal to
    the reference's `np.real(trace(scipy.linalg.sqrtm(...)))` to ~1e-9 relative (tests/test_host_logic.py);
  * the generator is this package's HIP path (`sd_util.sid_sd_sampler` with `return_images=True`: UNet + VAE decoder
    kernels); the feature detectors are PLUGGABLE callables -- the reference downloads a TorchScript Inception-v3
    (`inception-2015-12-05.pt`) and pickled open_clip models, neither of which exists offline.  `load_detector(path)`
    accepts exactly those files (torch.jit / pickle) when a deployment has them; the real-set statistics come from a cached
    `.npz` (`mu`, `sigma`) or are computed from the image set of `--data` with the same detector (`dataset_feature_stats`,
    metrics/sid_metric_utils.py:266-280) and cached as `<run_dir>/real_stats.npz`;
  * precision / recall (metrics/sid_precision_recall.py, Kynkaanniemi et al.; the SAME Inception detector as FID) keeps every
    feature vector on the device and runs on the `sidlsg_pr_*` kernels: the k-th neighbour radius and the membership test are
    reductions inside the fp16 MFMA distance contraction, so no N x N matrix is formed, let alone copied to the host as the
    reference does.  The distance is computed to fp32 accuracy and rounded to fp16 once; the reference's fp16 `cdist` is not
    correctly rounded, so single distances differ by an fp16 ulp (tests/test_gpu_pr.py pins what follows from that).
  * KID and CMMD are not in the reference: both are sums of a kernel function over all pairs of feature vectors, formed by
    `ops.pair_kernel_sums` (fp32 operands on the MFMA, fp64 sums in a fixed order, no N x N matrix); see the section above the registry.
  * the Inception-v3 itself runs on this package's kernels when its weights come as a state dict (sid_lsg_amd.inception; or the seeded
    'random:inception-v3'), and the Inception Score (`compute_is`, not in the reference either) reads its class probabilities.
Only the precision / recall and pair-sum kernels are hot; the rest is host logic.
"""
import json
import os
import pickle
import time

import numpy as np
import torch

from . import distributed as dist
from .dnnlib_util import EasyDict


# ------------------------------------------------------------------------------------------------
class FeatureStats:
    """Running mean / covariance of feature vectors (metrics/sid_metric_utils.py:112-188), accumulated in fp64 on `device`."""

    def __init__(self, capture_all=False, capture_mean_cov=False, max_items=None, device=None, keep_on_device=False):
        self.capture_all, self.capture_mean_cov, self.max_items = capture_all, capture_mean_cov, max_items
        self.keep_on_device = keep_on_device        # capture_all: the features stay where they were computed (precision / recall)
        self.device = torch.device(device) if device is not None else None
        self.num_items, self.num_features = 0, None
        self.all_features, self.raw_mean, self.raw_cov = None, None, None

    def set_num_features(self, num_features, device):
        if self.num_features is not None:
            assert num_features == self.num_features
            return
        self.num_features = num_features
        self.device = self.device or device
        self.all_features = []
        self.raw_mean = torch.zeros(num_features, dtype=torch.float64, device=self.device)
        self.raw_cov = torch.zeros(num_features, num_features, dtype=torch.float64, device=self.device)

    def is_full(self):
        return self.max_items is not None and self.num_items >= self.max_items

    def append(self, x):
        x = torch.as_tensor(x)
        assert x.ndim == 2
        if self.max_items is not None and self.num_items + x.shape[0] > self.max_items:
            if self.num_items >= self.max_items:
                return
            x = x[:self.max_items - self.num_items]
        self.set_num_features(x.shape[1], x.device)
        self.num_items += x.shape[0]
        x = x.to(self.device, torch.float32)          # the reference rounds features to fp32 before accumulating in fp64
        if self.capture_all:
            self.all_features.append(x if self.keep_on_device else x.cpu())
        if self.capture_mean_cov:
            x64 = x.to(torch.float64)
            self.raw_mean += x64.sum(0)
            self.raw_cov += x64.t() @ x64

    append_torch = append

    def merge_ranks(self, group=None):
        """Sum the accumulators over the ranks of the process group (each rank appended its own shard of the samples)."""
        world = dist.get_world_size()
        if world == 1:
            return self
        n = torch.tensor([float(self.num_items)], dtype=torch.float64, device=self.device)
        torch.distributed.all_reduce(n, group=group)
        if self.capture_all:
            # rank r holds the samples r, r + world, ...: ONE all_gather of the (equally padded) shards, interleaved back into
            # sample order, so every rank ends with the same [num_items, F] matrix
            assert self.keep_on_device, 'captured features are exchanged on the device'
            mine = torch.cat(self.all_features, 0)
            total = int(n.item())
            per = (total + world - 1) // world
            shard = torch.zeros(per, mine.shape[1], dtype=mine.dtype, device=mine.device)
            shard[:mine.shape[0]] = mine
            parts = [torch.empty_like(shard) for _ in range(world)]
            torch.distributed.all_gather(parts, shard, group=group)
            self.all_features = [torch.stack(parts, 1).reshape(per * world, -1)[:total]]
        if self.capture_mean_cov:
            for t in (self.raw_mean, self.raw_cov):
                torch.distributed.all_reduce(t, group=group)
        self.num_items = int(n.item())
        return self

    def get_all_torch(self):
        assert self.capture_all
        return torch.cat(self.all_features, 0)

    def get_all(self):
        return self.get_all_torch().cpu().numpy()

    def get_mean_cov(self):
        assert self.capture_mean_cov and self.num_items > 0
        mean = self.raw_mean / self.num_items
        cov = self.raw_cov / self.num_items - torch.outer(mean, mean)
        return mean.cpu().numpy(), cov.cpu().numpy()

    def save(self, path):
        mu, sigma = self.get_mean_cov()
        np.savez(path, mu=mu, sigma=sigma, num_items=self.num_items)


def frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real):
    """|mu_g - mu_r|^2 + tr(S_g + S_r - 2 (S_g S_r)^1/2)   (metrics/sid_fid_and_clip.py:65-67).
    tr((S_g S_r)^1/2) = sum_i sqrt(lambda_i(S_r^1/2 S_g S_r^1/2)): both factors are symmetric PSD, so two fp64 `eigh`
    give it without a general matrix square root."""
    mu_g, mu_r = (torch.as_tensor(np.asarray(m), dtype=torch.float64) for m in (mu_gen, mu_real))
    s_g, s_r = (torch.as_tensor(np.asarray(s), dtype=torch.float64) for s in (sigma_gen, sigma_real))
    w, v = torch.linalg.eigh((s_r + s_r.t()) * 0.5)
    root_r = (v * w.clamp_min(0).sqrt()) @ v.t()
    mid = root_r @ ((s_g + s_g.t()) * 0.5) @ root_r
    tr_sqrt = torch.linalg.eigvalsh((mid + mid.t()) * 0.5).clamp_min(0).sqrt().sum()
    return float((mu_g - mu_r).square().sum() + torch.trace(s_g) + torch.trace(s_r) - 2.0 * tr_sqrt)


def clip_score_from_features(features):
    """features [N, 2F] = image | text halves (already normalised by the detector): mean cosine (sid_metric_utils.py:503-504)."""
    f = torch.as_tensor(features)
    img, txt = f.tensor_split((f.shape[1] // 2,), 1)
    return float((img * txt).sum(-1).mean())


# ------------------------------------------------------------------------------------------------
def is_clip_spec(path):
    """A CLIP model this package builds itself: a local directory in the Hugging Face layout (config.json, model.safetensors,
    vocab.json, merges.txt) or 'random:clip-<arch>' (sid_lsg_amd.clip)."""
    return isinstance(path, (str, os.PathLike)) and (str(path).lower().startswith('random:clip-') or os.path.isfile(os.path.join(str(path), 'config.json')))


def is_inception_spec(path):
    """'random:inception-v3[:seed]': the seeded Inception-v3 this package builds itself (sid_lsg_amd.inception)."""
    return isinstance(path, str) and (path.lower() == 'random:inception-v3' or path.lower().startswith('random:inception-v3:'))


def load_detector(path, device):
    """A feature detector file of the reference's kinds: TorchScript (`inception-2015-12-05.pt`, called as
    `detector(uint8 NCHW images, return_features=True)`) or a pickled module (open_clip / CLIP wrappers, called with
    `texts=..., div255=True`).  Offline there are none: callers may pass any callable instead.  A CLIP directory (is_clip_spec) gives
    a `clip.HipCLIPDetector` with the wrappers' call contract: the image tower on the HIP kernels.  The Inception-v3 as a
    torch.save'd state dict in torchvision / pytorch-fid key names, or 'random:inception-v3[:seed]', gives an
    `inception.HipInceptionV3` with the TorchScript detector's call contract: the whole network on the HIP kernels."""
    if callable(path):
        return path
    if is_clip_spec(path):
        from .clip import load_clip
        return load_clip(path, device)
    if is_inception_spec(path):
        from .inception import load_inception
        return load_inception(path, device)
    if not path or not os.path.isfile(path):
        raise FileNotFoundError(f'feature detector {path!r} not found: FID / CLIP metrics need the Inception / CLIP files the reference '
                                'downloads (metrics/sid_fid_and_clip.py:36, sid_metric_utils.py:456); pass a local file or a callable')
    from . import inception
    state_dict = inception.load_state_dict_file(path)       # None for a TorchScript archive or a pickled module
    if state_dict is not None:
        return inception.HipInceptionV3(state_dict, device)
    try:
        return torch.jit.load(path, map_location=device).eval()
    except Exception:
        with open(path, 'rb') as f:
            return pickle.load(f).to(device).eval()


_LANCZOS_CACHE = {}


def _lanczos_coefficients(in_size, out_size):
    """The integer filter bank of Pillow's 8-bit LANCZOS resampling, [out_size, in_size] int64 (Pillow src/libImaging/Resample.c:
    `precompute_coeffs` with the a = 3 windowed sinc -- support 3 * max(scale, 1) input pixels around (x + 0.5) * scale, weights
    normalised to sum 1 -- then `normalize_coeffs_8bpc`: round-half-away to 22 fractional bits)."""
    import math
    key = (in_size, out_size)
    if key in _LANCZOS_CACHE:
        return _LANCZOS_CACHE[key]
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 3.0 * fscale
    K = np.zeros((out_size, in_size), dtype=np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        arg = (np.arange(xmin, xmax) - center + 0.5) / fscale
        with np.errstate(invalid='ignore', divide='ignore'):
            sinc = lambda t: np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))      # noqa: E731
            w = np.where((arg >= -3.0) & (arg < 3.0), sinc(arg) * sinc(arg / 3.0), 0.0)
        tot = w.sum()
        if tot != 0:
            w = w / tot
        K[xx, xmin:xmax] = np.where(w < 0, np.trunc(-0.5 + w * (1 << 22)), np.trunc(0.5 + w * (1 << 22))).astype(np.int64)
    _LANCZOS_CACHE[key] = K
    return K


_BICUBIC_CACHE = {}
PIL_PRECISION_BITS = 22


def _bicubic_coefficients(in_size, out_size):
    """The integer filter bank of Pillow's 8-bit BICUBIC resampling (Resample.c `precompute_coeffs` with the a = -0.5 cubic, support
    2 * max(scale, 1) around (x + 0.5) * scale, the window [int(centre - support + 0.5), int(centre + support + 0.5)) clipped to the
    image, weights summed in window order and normalised to sum 1; then `normalize_coeffs_8bpc`: round-half-away to 22 fractional
    bits) -> (bounds int32 [out_size, 2] = (first input pixel, taps), coefficients int32 [out_size, ksize], zero behind the taps).
    in_size == out_size: Pillow takes no pass over that side; the bank is then the one tap 1 << 22, which the integer pass maps to
    the pixel itself."""
    key = (in_size, out_size)
    if key in _BICUBIC_CACHE:
        return _BICUBIC_CACHE[key]
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size), np.ones(out_size, dtype=np.int64)], 1).astype(np.int32)
        coeffs = np.full((out_size, 1), 1 << PIL_PRECISION_BITS, dtype=np.int32)
        _BICUBIC_CACHE[key] = (bounds, coeffs)
        return bounds, coeffs
    import math
    a = -0.5

    def cubic(x):
        x = -x if x < 0.0 else x
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    one = float(1 << PIL_PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [cubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:                          # Pillow's own order: a pairwise sum can differ in the last bit
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        coeffs[xx, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
    _BICUBIC_CACHE[key] = (bounds, coeffs)
    return bounds, coeffs


def pil_resized_size(H, W, size):
    """(height, width) torchvision's `Resize(size)` gives a PIL image of H x W: the shorter side becomes `size`, the longer one
    int(size * long / short)."""
    return (size, int(size * W / H)) if H <= W else (int(size * H / W), size)


def pil_crop_offset(side, size):
    """Where torchvision's `CenterCrop(size)` starts on a side of length `side`: Python's round, half to even."""
    return int(round((side - size) / 2.0))


def pil_crop_plan(H, W, size, patch=None):
    """open_clip's validation transform `Resize(size, BICUBIC)` + `CenterCrop(size)` of an H x W image as the two coefficient banks
    restricted to the crop, what sidlsg_pil_patches_u8 takes: dict(hbounds [size, 2], hcoef [size, hk], vbounds, vcoef (int32),
    resized=(h, w), crop=(top, left), band_rows = the most source rows the vertical windows of `patch` consecutive output rows span)."""
    h, w = pil_resized_size(H, W, size)
    top, left = pil_crop_offset(h, size), pil_crop_offset(w, size)
    hb, hc = _bicubic_coefficients(W, w)
    vb, vc = _bicubic_coefficients(H, h)
    hb, hc, vb, vc = (np.ascontiguousarray(t) for t in (hb[left:left + size], hc[left:left + size], vb[top:top + size], vc[top:top + size]))
    plan = dict(hbounds=hb, hcoef=hc, vbounds=vb, vcoef=vc, resized=(h, w), crop=(top, left))
    if patch is not None:
        first = vb[0::patch, 0]
        last = vb[patch - 1::patch]
        plan['band_rows'] = int((last[:, 0] + last[:, 1] - first).max())
    return plan


def pil_resize_crop_u8(image_u8, size):
    """uint8 [C, H, W] (numpy) -> uint8 [C, size, size]: Pillow's `Image.resize(BICUBIC)` of the shorter side to `size` and the centre
    crop, restated in integers on the host (the arithmetic sidlsg_pil_patches_u8 runs; pinned against Pillow in
    tests/test_hps_host.py).  Horizontal pass, then vertical, each clip8((sum + 2^21) >> 22)."""
    image_u8 = np.asarray(image_u8)
    C, H, W = image_u8.shape
    plan = pil_crop_plan(H, W, size)
    half = 1 << (PIL_PRECISION_BITS - 1)

    def one_pass(src, bounds, coeffs):          # along the last axis
        out = np.empty(src.shape[:-1] + (len(bounds),), dtype=np.uint8)
        s = src.astype(np.int64)
        for x, (x0, n) in enumerate(bounds):
            acc = (s[..., x0:x0 + n] * coeffs[x, :n].astype(np.int64)).sum(-1) + half
            out[..., x] = np.clip(acc >> PIL_PRECISION_BITS, 0, 255)
        return out
    t = one_pass(image_u8, plan['hbounds'], plan['hcoef'])                                     # [C, H, size]
    return one_pass(t.transpose(0, 2, 1), plan['vbounds'], plan['vcoef']).transpose(0, 2, 1)    # [C, size, size]


def resize_for_detector(images_u8, size=256):
    """uint8 NCHW -> uint8 NCHW at size x size with the arithmetic of the reference's `resize_images_in_tensor`
    (sid_metric_utils.py:353-375: per image `PIL.Image.resize((256, 256), Image.LANCZOS)`, back to uint8) -- on the device, for the
    whole batch: Pillow's two passes (horizontal, then vertical, each rounded to 8 bits) with its 22-bit fixed-point coefficients.
    Sums of 8-bit pixels times 22-bit integers are exact in fp64, so two fp64 GEMMs reproduce the integer pipeline bit for bit
    (pinned against PIL itself: tests/golden/metrics_ref.npz, tests/test_host_logic.py)."""
    if images_u8.dtype != torch.uint8 or images_u8.ndim != 4:
        raise ValueError('resize_for_detector: uint8 NCHW images')
    H, W = images_u8.shape[-2:]
    if H == size and W == size:
        return images_u8
    dev = images_u8.device
    kh = torch.from_numpy(_lanczos_coefficients(W, size)).to(dev, torch.float64)
    kv = torch.from_numpy(_lanczos_coefficients(H, size)).to(dev, torch.float64)
    half, one = float(1 << 21), float(1 << 22)
    t = torch.matmul(images_u8.to(torch.float64), kh.t())                      # [N, C, H, size]
    t = torch.floor((t + half) / one).clamp_(0, 255)
    t = torch.matmul(kv, t)                                                    # [N, C, size, size]
    t = torch.floor((t + half) / one).clamp_(0, 255)
    return t.to(torch.uint8)


class _PromptList:
    """A list of prompts with the dataset item contract `(image, text)` (for callers that hold plain strings)."""

    def __init__(self, prompts):
        self.prompt_list = list(prompts)

    def __len__(self):
        return len(self.prompt_list)

    def __getitem__(self, i):
        return None, self.prompt_list[i]


class MetricOptions:
    """What a metric needs (reference: sid_metric_utils.MetricOptions): a generator `G(latents=, contexts=, init_timesteps=)`
    returning images in [-1, 1], the prompt source, the detectors, the real-set statistics.
    Prompt source: `dataset_kwargs` (what the reference passes, sid_training_loop.py:636: the evaluation caption set of
    `--data`, built by class name) or `dataset` (an object with that item contract) or `prompts` (a list of strings).  The
    evaluation order is the reference's: `InfiniteSampler(dataset, rank, num_gpus, seed=0)` (sid_metric_utils.py:420)."""

    def __init__(self, G, prompts=None, resolution=512, init_timestep=625, detector=None, real_stats=None, open_clip_detector=None,
                 clip_score_fn=None, device=None, seed=0, batch_gen=4, detector_size=256, progress=None, dataset_kwargs=None,
                 dataset=None, run_dir=None, metric_clip_path=None, metric_hps_path=None, hps_prompts=None, hps_arch=None, hps_tokenizer=None,
                 hps_detector=None, metric_cmmd_clip_path=None, metric_lpips_vgg=None, metric_lpips_lin=None, lpips_detector=None):
        from .dnnlib_util import construct_class_by_name
        self.metric_cmmd_clip_path = metric_cmmd_clip_path      # --metric_cmmd_clip_path: the CLIP image tower behind `cmmd*`
        # --metric_lpips_vgg / --metric_lpips_lin: the LPIPS-VGG weights behind `lpipsdiv*` (or a ready fidelity.HipLPIPS)
        self.metric_lpips_vgg, self.metric_lpips_lin, self.lpips_detector = metric_lpips_vgg, metric_lpips_lin, lpips_detector
        self.run_dir = run_dir
        if dataset is None and dataset_kwargs:
            dataset = construct_class_by_name(**dataset_kwargs)
        if dataset is None:
            if prompts is None and hps_prompts is not None:
                prompts = []                         # hpsv2 brings its own prompts
            if prompts is None:
                raise ValueError('metrics need a prompt source: dataset_kwargs, dataset or prompts')
            dataset = _PromptList(prompts)
        self.dataset = dataset
        # --metric_hps_path / --hps_prompts / --hps_arch / --hps_tokenizer: the scorer and the benchmark prompts of `hpsv2`
        self.metric_hps_path, self.hps_prompts, self.hps_arch, self.hps_tokenizer = metric_hps_path, hps_prompts, hps_arch, hps_tokenizer
        self.hps_detector = hps_detector            # a ready clip.HipCLIPDetector instead of the checkpoint (callers that hold one)
        self.G, self.resolution, self.init_timestep = G, resolution, init_timestep
        self.detector, self.real_stats, self.open_clip_detector, self.clip_score_fn = detector, real_stats, open_clip_detector, clip_score_fn
        self.metric_clip_path = metric_clip_path        # --metric_clip_path: the detector behind `clipscore30k` when clip_score_fn is None
        self.device = torch.device(device if device is not None else 'cuda')
        self.seed, self.batch_gen, self.detector_size, self.progress = seed, batch_gen, detector_size, progress
        self.rank, self.num_gpus = dist.get_rank(), dist.get_world_size()


def row_cosines(detector):
    """`clip_score_fn(images_u8, texts) -> [B]` of a CLIP detector: its own `scores` (HipCLIPDetector), else the row dot product
    of the image | text halves it returns."""
    if hasattr(detector, 'scores'):
        return detector.scores

    def fn(images, texts):
        img, txt = torch.as_tensor(detector(images, texts=texts, div255=True)).float().chunk(2, 1)
        return (img * txt).sum(-1)
    return fn


def _caption(dataset, i):
    """Caption i without decoding the image next to it."""
    return dataset.caption(i) if hasattr(dataset, 'caption') else dataset[i][1]


def dataset_feature_stats(opts, max_items=None, capture_all=False):
    """Detector features of the real images (compute_feature_stats_for_dataset, metrics/sid_metric_utils.py:266-280): the first
    min(len, max_items) items of `opts.dataset`, rank-strided, to the device as uint8 exactly as stored (no resize), grey -> 3
    channels, through the detector.  -> FeatureStats holding mean / covariance, or (capture_all) every feature vector in item
    order ON THE DEVICE; ranks are merged, so every rank returns the same statistics."""
    dataset = opts.dataset
    if not getattr(dataset, 'has_images', False):
        raise ValueError('real-set features need an image dataset (--data: a directory of images with .txt captions; '
                         'sid_lsg_amd.data.ImageCaptionDataset), not a caption list')
    num_items = len(dataset) if max_items is None else min(len(dataset), max_items)
    if num_items < opts.num_gpus:
        raise ValueError(f'{num_items} real images for {opts.num_gpus} ranks: every rank needs at least one')
    detector = load_detector(opts.detector, opts.device)
    stats = FeatureStats(capture_all=capture_all, capture_mean_cov=not capture_all, device=opts.device, keep_on_device=capture_all)
    mine = list(range(opts.rank, num_items, opts.num_gpus))
    batch = []

    def flush():
        if batch:
            images = torch.stack(batch).to(opts.device)
            if images.shape[1] == 1:
                images = images.repeat(1, 3, 1, 1)
            with torch.no_grad():
                stats.append(detector(images, return_features=True))
            batch.clear()
    for n, i in enumerate(mine):
        image = dataset[i][0]
        if batch and (len(batch) == 64 or image.shape != batch[0].shape):      # a batch is a run of equally sized images
            flush()
        batch.append(image)
        if opts.progress is not None and n % 64 == 0:
            opts.progress(n * opts.num_gpus, num_items)
    flush()
    return stats.merge_ranks()


def generator_feature_stats(opts, num_gen, compute_clip=False, capture_all=False):
    """sid_metric_utils.py:412-510: this rank's share of `num_gen` samples -- prompts in the order of the reference's
    `InfiniteSampler(dataset, rank, num_gpus, seed=0)` (shuffled, rank-strided; :420), z ~ N(0, I) from a per-rank generator --
    through G, the detector and (optionally) the CLIP detectors."""
    from .data import InfiniteSampler
    order = iter(InfiniteSampler(opts.dataset, rank=opts.rank, num_replicas=opts.num_gpus, seed=0))
    detector = load_detector(opts.detector, opts.device)
    oc = load_detector(opts.open_clip_detector, opts.device) if (compute_clip and opts.open_clip_detector is not None) else None
    clip_score_fn = opts.clip_score_fn if compute_clip else None
    if compute_clip and clip_score_fn is None and opts.metric_clip_path is not None:
        # each detector is loaded once per metric call; one model given under both names is loaded once
        same = oc is not None and isinstance(opts.open_clip_detector, str) and opts.open_clip_detector == opts.metric_clip_path
        clip_score_fn = row_cosines(oc if same else load_detector(opts.metric_clip_path, opts.device))
    stats = FeatureStats(capture_mean_cov=not capture_all, capture_all=capture_all, keep_on_device=capture_all, max_items=None, device=opts.device)
    gen = torch.Generator(device=opts.device).manual_seed(opts.seed * opts.num_gpus + opts.rank)
    lat = opts.resolution // 8
    mine = list(range(opts.rank, num_gen, opts.num_gpus))          # global sample indices of this rank
    oc_scores, clip_scores = [], []
    for i in range(0, len(mine), opts.batch_gen):
        idx = mine[i:i + opts.batch_gen]
        texts = [_caption(opts.dataset, next(order)) for _ in idx]
        z = torch.randn([len(idx), 4, lat, lat], device=opts.device, generator=gen)
        with torch.no_grad():
            img = opts.G(latents=z, contexts=texts, init_timesteps=opts.init_timestep * torch.ones(len(idx), device=opts.device, dtype=torch.long))
        img = (img * 127.5 + 128).clamp(0, 255).to(torch.uint8)
        if img.shape[1] == 1:
            img = img.repeat(1, 3, 1, 1)
        if opts.detector_size is not None:      # None: the detector resamples the images itself (compute_cmmd)
            img = resize_for_detector(img, opts.detector_size)
        with torch.no_grad():
            stats.append(detector(img, return_features=True))
            if compute_clip:
                if clip_score_fn is not None:
                    clip_scores.append(torch.as_tensor(clip_score_fn(img, texts)).float().flatten().cpu())
                if oc is not None:
                    oc_scores.append(torch.tensor([clip_score_from_features(oc(img, texts=texts, div255=True))] * len(idx)))
        if opts.progress is not None:
            opts.progress(stats.num_items * opts.num_gpus, num_gen)
    stats.merge_ranks()

    def mean_over_ranks(parts):
        if not parts:
            return float('nan')
        v = torch.cat(parts).double()
        t = torch.tensor([float(v.sum()), float(v.numel())], dtype=torch.float64, device=opts.device)
        if opts.num_gpus > 1:
            torch.distributed.all_reduce(t)
        return float(t[0] / t[1])
    return stats, mean_over_ranks(oc_scores), mean_over_ranks(clip_scores)


REAL_STATS_FILE = 'real_stats.npz'


def load_real_stats(real_stats, opts=None):
    """(mu, sigma) of the real set: a cached .npz / .pkl of the reference's FeatureStats dict, or a (mu, sigma) pair.  None with
    an image dataset in `opts`: `<opts.run_dir>/real_stats.npz` when a previous tick or run left it, else computed from the images
    (dataset_feature_stats) and cached there in the same layout, ready to be passed as --data_stat."""
    if real_stats is None and opts is not None and getattr(opts.dataset, 'has_images', False):
        cache = os.path.join(opts.run_dir, REAL_STATS_FILE) if opts.run_dir else None
        have = torch.tensor([1.0 if (cache and opts.rank == 0 and os.path.isfile(cache)) else 0.0], device=opts.device)
        if opts.num_gpus > 1:
            torch.distributed.broadcast(have, src=0)         # all ranks agree (the file is rank 0's)
        if float(have) != 0:
            return load_real_stats(cache)
        stats = dataset_feature_stats(opts)
        if cache and opts.rank == 0:
            os.makedirs(opts.run_dir, exist_ok=True)
            tmp = cache + '.tmp.npz'
            stats.save(tmp)
            os.replace(tmp, cache)
        return stats.get_mean_cov()
    if isinstance(real_stats, (tuple, list)):
        return np.asarray(real_stats[0]), np.asarray(real_stats[1])
    if isinstance(real_stats, str) and real_stats.endswith('.npz'):
        d = np.load(real_stats)
        return d['mu'], d['sigma']
    if isinstance(real_stats, str):
        with open(real_stats, 'rb') as f:
            s = pickle.load(f)
        mean = s['raw_mean'] / s['num_items']
        return mean, s['raw_cov'] / s['num_items'] - np.outer(mean, mean)
    raise ValueError('real_stats: a (mu, sigma) pair, a .npz with mu / sigma, or a pickled FeatureStats of the reference')


def compute_fid_and_clip(opts, num_gen, compute_clip=False):
    """metrics/sid_fid_and_clip.py:32-74."""
    mu_real, sigma_real = load_real_stats(opts.real_stats, opts)
    stats, open_clip_score, clip_score = generator_feature_stats(opts, num_gen, compute_clip)
    mu_gen, sigma_gen = stats.get_mean_cov()
    fid = frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real)
    return (fid, open_clip_score, clip_score) if compute_clip else fid


def compute_pr(opts, max_real, num_gen, nhood_size):
    """Precision and recall of Kynkaanniemi et al. (metrics/sid_precision_recall.py:36-66): a generated sample counts towards
    precision when it lies within the k-th neighbour radius of some real feature vector, a real one towards recall when it lies
    within that of some generated one.  Features rounded to fp16 as the reference does (:48, :52); radius and membership on the
    sidlsg_pr_* kernels.  Every rank holds all features after the gather and computes the same two numbers."""
    from . import ops
    real = dataset_feature_stats(opts, max_items=max_real, capture_all=True).get_all_torch()
    gen = generator_feature_stats(opts, num_gen, capture_all=True)[0].get_all_torch()
    real, gen = (f.to(opts.device, torch.float16).contiguous() for f in (real, gen))
    results = {}
    for name, manifold, probes in (('precision', real, gen), ('recall', gen, real)):
        k = nhood_size
        if manifold.shape[0] <= k:       # the reference's kthvalue raises here; the smoke-sized pr_test takes the farthest member
            k = manifold.shape[0] - 1
            dist.print0(f'WARNING: precision / recall: {manifold.shape[0]} features for nhood_size {nhood_size}: using k = {k}')
        radius = ops.pr_kth_radius(manifold, k)
        results[name] = float(ops.pr_member(probes, manifold, radius).to(torch.float64).mean())       # the exact share: count / n
    return results['precision'], results['recall']


# ------------------------------------------------------------------------------------------------
# KID (Binkowski et al., "Demystifying MMD GANs"; `kid50k_full` of the StyleGAN2-ADA / StyleGAN3 metric registry) and CMMD
# (Jayasumana et al. 2024, "Rethinking FID").  Both are three sums over all pairs of a kernel function of feature dot products,
# which ops.pair_kernel_sums forms on the f32 MFMA and adds in fp64; the functions below are the arithmetic around those sums.
# They restate the published formulas and are not pinned against those packages.
KID_NUM_SUBSETS, KID_MAX_SUBSET_SIZE = 100, 1000
CMMD_SIGMA, CMMD_SCALE = 10.0, 1000.0


def kid_subsets(n_gen, n_real, num_subsets=KID_NUM_SUBSETS, max_subset_size=KID_MAX_SUBSET_SIZE, seed=0):
    """(ix, iy) int32 [num_subsets, m], m = min(n_gen, n_real, max_subset_size): the rows of the generated and of the real features
    each subset uses.  StyleGAN's kernel_inception_distance.py draws, per subset, `choice(n_gen, m, replace=False)` and then
    `choice(n_real, m, replace=False)` from numpy's global generator; here from RandomState(seed), in that order."""
    m = min(int(n_gen), int(n_real), int(max_subset_size))
    if m < 1 or num_subsets < 1:
        raise ValueError(f'kid_subsets: {n_gen} generated and {n_real} real features in {num_subsets} subsets of at most {max_subset_size}')
    rnd = np.random.RandomState(seed)
    ix = np.empty((num_subsets, m), dtype=np.int32)
    iy = np.empty((num_subsets, m), dtype=np.int32)
    for s in range(num_subsets):
        ix[s] = rnd.choice(n_gen, m, replace=False)
        iy[s] = rnd.choice(n_real, m, replace=False)
    return ix, iy


def kid_from_sums(sums, m):
    """[S, 5] sums (Sxx, Syy, Sxy, Txx, Tyy) of the cubic kernel (x.y / F + 1)^3 over subsets of m rows -> KID, in fp64:
    t_s = ((Sxx - Txx) + (Syy - Tyy)) / (m - 1) - 2 Sxy / m;  KID = mean_s(t_s) / m   (the unbiased estimator: no i == j pairs).
    m = 1 leaves no pair i != j: NaN, the 0 / 0 of the published code (the one-sample `kid_test` of a smoke run)."""
    if m < 2:
        return float('nan')
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 5)
    t = ((s[:, 0] - s[:, 3]) + (s[:, 1] - s[:, 4])) / (m - 1) - 2.0 * s[:, 2] / m
    return float(t.mean() / m)


def cmmd_from_sums(sums, nx, ny, scale=CMMD_SCALE):
    """[5] (or [1, 5]) sums of 1 - k, k = exp(-|a - b|^2 / (2 sigma^2)), over all pairs, the diagonal included -> scale * MMD^2, in
    fp64: mean(k_xx) + mean(k_yy) - 2 mean(k_xy) = 2 Sxy / (nx ny) - Sxx / nx^2 - Syy / ny^2  (the biased V-statistic of the
    published CMMD code; the ones cancel exactly instead of in floating point)."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1)
    return float(scale * (2.0 * s[2] / (float(nx) * float(ny)) - s[0] / float(nx) ** 2 - s[1] / float(ny) ** 2))


def _features_f32(t, device):
    return torch.as_tensor(t).to(device, torch.float32).contiguous()


def kid_from_features(real, gen, num_subsets=KID_NUM_SUBSETS, max_subset_size=KID_MAX_SUBSET_SIZE, seed=0):
    """KID between [n_real, F] and [n_gen, F] fp32 features on the device: the subsets are index lists read by one launch."""
    from . import ops
    ix, iy = kid_subsets(gen.shape[0], real.shape[0], num_subsets, max_subset_size, seed)
    sums = ops.pair_kernel_sums(gen, real, ops.PAIR_KERNEL_POLY3, 1.0 / gen.shape[1], 1.0,
                                torch.from_numpy(ix).to(gen.device), torch.from_numpy(iy).to(gen.device))
    return kid_from_sums(sums.cpu().numpy(), ix.shape[1])


def cmmd_from_features(real, gen, sigma=CMMD_SIGMA, scale=CMMD_SCALE):
    """CMMD between [n_real, F] and [n_gen, F] fp32 (L2-normalised CLIP) embeddings on the device."""
    from . import ops
    sums = ops.pair_kernel_sums(real, gen, ops.PAIR_KERNEL_RBF, 1.0 / (2.0 * sigma * sigma))
    return cmmd_from_sums(sums.cpu().numpy(), real.shape[0], gen.shape[0], scale)


def compute_kid(opts, max_real, num_gen, num_subsets=KID_NUM_SUBSETS, max_subset_size=KID_MAX_SUBSET_SIZE):
    """KID of `num_gen` generated images against the first `max_real` real ones: the Inception detector and the 256 x 256 resize of
    FID, fp32 features kept on the device (as compute_pr keeps them).  Every rank holds all features and computes the same number."""
    real = dataset_feature_stats(opts, max_items=max_real, capture_all=True).get_all_torch()
    gen = generator_feature_stats(opts, num_gen, capture_all=True)[0].get_all_torch()
    if min(real.shape[0], gen.shape[0]) < 2:
        dist.print0(f'WARNING: KID: {real.shape[0]} real and {gen.shape[0]} generated features: subsets of one feature have no pair, the result is NaN')
    return kid_from_features(_features_f32(real, opts.device), _features_f32(gen, opts.device), num_subsets, max_subset_size)


# Inception Score (Salimans et al. 2016; `is50k` of the StyleGAN3 metric registry, metrics/inception_score.py there): restated from
# the published source, not pinned against that package.
def is_from_probabilities(probs, num_splits=10):
    """[N, C] class probabilities -> (mean, population std) over `num_splits` contiguous splits of
    exp(mean_i sum_c p_ic (log p_ic - log mean_i p_ic)), in fp64 (0 log 0 = 0).  Split s holds the rows
    s * N // num_splits .. (s + 1) * N // num_splits - 1.  Evaluated in base 2 (2^(.. log2 ..), the same number): one-hot rows spread
    evenly over K = 2^j classes then score K exactly, where exp(log K) is an ulp off."""
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim != 2 or num_splits < 1 or p.shape[0] < num_splits:
        raise ValueError(f'inception score: {p.shape} probabilities in {num_splits} splits')
    scores = []
    for s in range(num_splits):
        part = p[s * p.shape[0] // num_splits:(s + 1) * p.shape[0] // num_splits]
        with np.errstate(divide='ignore', invalid='ignore'):
            kl = part * (np.log2(part) - np.log2(part.mean(axis=0, keepdims=True)))
        scores.append(np.exp2(np.where(part > 0, kl, 0.0).sum(axis=1).mean()))
    return float(np.mean(scores)), float(np.std(scores))


class _ProbabilityDetector:
    """The detector as compute_is reads it: class probabilities without fc's bias, through the `return_features` call of the loops."""

    def __init__(self, detector):
        self.detector = detector

    def __call__(self, images, return_features=True):
        return self.detector(images, no_output_bias=True)


def is_options(opts):
    """`opts` with the detector's probabilities in place of its features."""
    import copy
    o = copy.copy(opts)
    o.detector = _ProbabilityDetector(load_detector(opts.detector, opts.device))
    return o


def compute_is(opts, num_gen, num_splits=10):
    """Inception Score of `num_gen` generated images: the probabilities det(images, no_output_bias=True) after the 256 x 256 detector
    resize of FID, captured on the device, reduced in fp64.  Needs neither real images nor their statistics.  -> (mean, std)."""
    probs = generator_feature_stats(is_options(opts), num_gen, capture_all=True)[0].get_all_torch()
    return is_from_probabilities(probs.cpu().numpy(), num_splits)


class ClipEmbeddingDetector:
    """The image tower of a CLIP model with the detector call contract: uint8 images of any size -> F.normalize(image_embeds), fp32.
    The tower resamples H x W to its own R x R without a crop (preprocess='interpolate'), as the published CMMD code does."""

    def __init__(self, path, device):
        from .clip import load_clip
        self.vision = load_clip(path, device, preprocess='interpolate').vision

    def __call__(self, images_u8, return_features=True):
        with torch.no_grad():
            return torch.nn.functional.normalize(self.vision(images_u8).float(), dim=-1)


def cmmd_options(opts):
    """`opts` with the CMMD detector in place of the Inception one and no resize in front of it."""
    import copy
    if not opts.metric_cmmd_clip_path:
        raise ValueError('cmmd needs --metric_cmmd_clip_path: a local CLIP directory in the Hugging Face layout (ViT-L/14-336 in the '
                         'published CMMD) or random:clip-<arch>')
    o = copy.copy(opts)
    o.detector = ClipEmbeddingDetector(opts.metric_cmmd_clip_path, opts.device)
    o.detector_size = None
    return o


def compute_cmmd(opts, max_real, num_gen):
    """CMMD of `num_gen` generated images against the first `max_real` real ones: both through the same CLIP image tower, straight
    from their own sizes (no 256 x 256 step).  Every rank holds all embeddings and computes the same number."""
    o = cmmd_options(opts)
    real = dataset_feature_stats(o, max_items=max_real, capture_all=True).get_all_torch()
    gen = generator_feature_stats(o, num_gen, capture_all=True)[0].get_all_torch()
    return cmmd_from_features(_features_f32(real, opts.device), _features_f32(gen, opts.device))


# ------------------------------------------------------------------------------------------------
_metric_dict = {}


def register_metric(fn):
    _metric_dict[fn.__name__] = fn
    return fn


def is_valid_metric(metric):
    return metric in _metric_dict


def list_valid_metrics():
    return list(_metric_dict.keys())


@register_metric
def fid30k_full(opts):
    return dict(fid30k_full=compute_fid_and_clip(opts, 30000), open_clipscore_30k=float('nan'), clipscore30k=float('nan'))


@register_metric
def fid_clip_30k_full(opts):
    fid, oc, cs = compute_fid_and_clip(opts, 30000, compute_clip=True)
    return dict(fid30k_full=fid, open_clipscore_30k=oc, clipscore30k=cs)


@register_metric
def fid_test(opts):
    return dict(fid30k_full=compute_fid_and_clip(opts, max(1, getattr(opts, 'num_test', 1))), open_clipscore_30k=float('nan'), clipscore30k=float('nan'))


@register_metric
def fid_clip_test(opts):
    fid, oc, cs = compute_fid_and_clip(opts, max(1, getattr(opts, 'num_test', 1)), compute_clip=True)
    return dict(fid30k_full=fid, open_clipscore_30k=oc, clipscore30k=cs)


@register_metric
def pr30k3_full(opts):
    precision, recall = compute_pr(opts, max_real=None, num_gen=30000, nhood_size=3)
    return dict(pr30k3_full_precision=precision, pr30k3_full_recall=recall)


@register_metric
def pr_test(opts):
    precision, recall = compute_pr(opts, max_real=None, num_gen=max(1, getattr(opts, 'num_test', 1)), nhood_size=3)
    return dict(pr30k3_full_precision=precision, pr30k3_full_recall=recall)


# registered here, behind the other metrics of the Inception detector: later entries keep their place at the end of the list
@register_metric
def is30k_full(opts):
    mean, std = compute_is(opts, num_gen=30000, num_splits=10)
    return dict(is30k_full_mean=mean, is30k_full_std=std)


@register_metric
def is_test(opts):
    mean, std = compute_is(opts, num_gen=max(1, getattr(opts, 'num_test', opts.batch_gen)), num_splits=1)
    return dict(is30k_full_mean=mean, is30k_full_std=std)


def compute_hps(opts, per_style):
    """HPSv2 benchmark score (the reference's generate_hpsv2.py + hpsv2.evaluate, sid_lsg_amd.hps): for each of the four styles,
    image i < per_style from prompt i of the style and the latent of torch.Generator(i) -- the same latents for every style --
    through G, uint8, PIL's JPEG encoder and decoder in memory (the scorer of the reference reads the .jpg files), scored by the
    open_clip checkpoint of --metric_hps_path on the HIP towers.  Rank-strided; every rank returns the same numbers."""
    from . import hps
    if not opts.hps_prompts or (opts.hps_detector is None and not opts.metric_hps_path):
        raise ValueError('hpsv2 needs --metric_hps_path (HPS_v2_compressed.pt, or any checkpoint in open_clip\'s layout) and --hps_prompts '
                         '(a directory with anime.json, concept-art.json, paintings.json, photo.json)')
    prompts = hps.benchmark_prompts(opts.hps_prompts)
    for style, p in prompts.items():
        if len(p) < per_style:
            raise ValueError(f'hpsv2: {style}.json of {opts.hps_prompts} has {len(p)} prompts, {per_style} are needed')
    det = opts.hps_detector
    if det is None:
        from .clip import load_open_clip
        det = load_open_clip(opts.metric_hps_path, opts.hps_tokenizer, opts.device, arch=opts.hps_arch or 'ViT-H-14')
    lat = opts.resolution // 8
    mine = list(range(opts.rank, per_style, opts.num_gpus))
    scores = {}
    for style in hps.STYLES:
        vals = []
        for i in range(0, len(mine), opts.batch_gen):
            idx = mine[i:i + opts.batch_gen]
            z = torch.stack([torch.randn([4, lat, lat], device=opts.device, generator=torch.Generator(opts.device).manual_seed(s)) for s in idx])
            texts = [prompts[style][s] for s in idx]
            with torch.no_grad():
                img = opts.G(latents=z, contexts=texts, init_timesteps=opts.init_timestep * torch.ones(len(idx), device=opts.device, dtype=torch.long))
            img = (img * 127.5 + 128).clamp(0, 255).to(torch.uint8)
            vals += hps.score(det, hps.jpeg_round_trip(img), texts).cpu().tolist()
            if opts.progress is not None:
                opts.progress(len(vals) * opts.num_gpus, per_style)
        scores[style] = vals
    res = hps.aggregate(hps.gather_scores(scores, list(range(per_style)), opts.rank, opts.num_gpus, opts.device))
    out = {f'hpsv2_{style}': res[style] for style in hps.STYLES}
    out['hpsv2'] = res['Average']
    return out


@register_metric
def hpsv2(opts):
    return compute_hps(opts, 800)


@register_metric
def hpsv2_test(opts):
    return compute_hps(opts, 16)


def compute_prompt_diversity(opts, num_prompts, per_prompt):
    """Intra-prompt diversity (sid_lsg_amd.diversity): for each of `num_prompts` prompts, `per_prompt` images from the latents of
    torch.Generator(p * per_prompt + j), j < per_prompt (compute_hps's rule), and the LPIPS-VGG of all their pairs from one VGG16
    pass (HipLPIPS.group_pairs).  The prompts are the first `num_prompts` of the order generator_feature_stats uses
    (InfiniteSampler(dataset, seed=0) over all ranks).  -> (mean over prompts of the mean pairwise LPIPS, mean over prompts of the
    smallest pair).  Prompts are rank-strided; every rank returns the same numbers.  Neither real images nor their statistics are read."""
    from . import fidelity
    from .data import InfiniteSampler
    lp = opts.lpips_detector
    if lp is None:
        if not opts.metric_lpips_vgg or not opts.metric_lpips_lin:
            raise ValueError('lpipsdiv needs --metric_lpips_vgg (a torchvision VGG16 state dict) and --metric_lpips_lin (the lpips package\'s '
                             f'vgg.pth), or {fidelity.RANDOM_PREFIX}[:seed] for both')
        lp = fidelity.load_lpips(opts.metric_lpips_vgg, opts.metric_lpips_lin, opts.device)
    if len(opts.dataset) < 1:
        raise ValueError('lpipsdiv needs a prompt source: dataset_kwargs, dataset or prompts')
    order = iter(InfiniteSampler(opts.dataset, rank=0, num_replicas=1, seed=0))
    captions = [_caption(opts.dataset, next(order)) for _ in range(num_prompts)]
    lat = opts.resolution // 8
    full = torch.zeros((num_prompts, 2), dtype=torch.float64, device=opts.device)
    for n, p in enumerate(range(opts.rank, num_prompts, opts.num_gpus)):
        imgs = []
        for i in range(0, per_prompt, opts.batch_gen):
            js = range(i, min(i + opts.batch_gen, per_prompt))
            z = torch.stack([torch.randn([4, lat, lat], device=opts.device, generator=torch.Generator(opts.device).manual_seed(p * per_prompt + j)) for j in js])
            with torch.no_grad():
                img = opts.G(latents=z, contexts=[captions[p]] * len(js), init_timesteps=opts.init_timestep * torch.ones(len(js), device=opts.device, dtype=torch.long))
            imgs.append((img * 127.5 + 128).clamp(0, 255).to(torch.uint8))
        pairs = lp.group_pairs(torch.cat(imgs), per_prompt)[0].cpu().tolist()
        total = 0.0
        for v in pairs:                                                                 # the pairs added in order, as diversity.score_groups does
            total += v
        full[p, 0], full[p, 1] = total / len(pairs), min(pairs)
        if opts.progress is not None:
            opts.progress((n + 1) * opts.num_gpus, num_prompts)
    if opts.num_gpus > 1:
        torch.distributed.all_reduce(full)
    rows = full.cpu().tolist()
    return sum(r[0] for r in rows) / num_prompts, sum(r[1] for r in rows) / num_prompts


@register_metric
def lpipsdiv1k_full(opts):
    mean, low = compute_prompt_diversity(opts, 1000, 8)
    return dict(lpipsdiv1k_full=mean, lpipsdiv1k_full_min=low)


@register_metric
def lpipsdiv_test(opts):
    mean, low = compute_prompt_diversity(opts, max(1, getattr(opts, 'num_test', 1)), 4)
    return dict(lpipsdiv_test=mean, lpipsdiv_test_min=low)


@register_metric
def kid30k_full(opts):
    return dict(kid30k_full=compute_kid(opts, max_real=None, num_gen=30000))


@register_metric
def kid_test(opts):
    return dict(kid30k_full=compute_kid(opts, max_real=None, num_gen=max(1, getattr(opts, 'num_test', 1))))


@register_metric
def cmmd30k_full(opts):
    return dict(cmmd30k_full=compute_cmmd(opts, max_real=None, num_gen=30000))


@register_metric
def cmmd_test(opts):
    return dict(cmmd30k_full=compute_cmmd(opts, max_real=None, num_gen=max(1, getattr(opts, 'num_test', 1))))


# metrics that read the real images themselves: --data_stat cannot stand in
NEEDS_IMAGES = ('pr30k3_full', 'pr_test', 'kid30k_full', 'kid_test', 'cmmd30k_full', 'cmmd_test')
HPS_METRICS = ('hpsv2', 'hpsv2_test')          # metrics that need neither the Inception detector nor real-set statistics
CMMD_METRICS = ('cmmd30k_full', 'cmmd_test')   # likewise: the CLIP image tower of --metric_cmmd_clip_path and the real images
IS_METRICS = ('is30k_full', 'is_test')         # the Inception detector alone: neither real images nor their statistics
LPIPSDIV_METRICS = ('lpipsdiv1k_full', 'lpipsdiv_test')      # --metric_lpips_vgg / --metric_lpips_lin alone: no Inception file, no statistics, no real images


def calc_metric(metric, **kwargs):
    """sid_metric_main.py:46-72: run one registered metric, return the decorated result dict."""
    if not is_valid_metric(metric):
        raise ValueError(f'unknown metric {metric!r}; valid: {list_valid_metrics()}')
    num_test = kwargs.pop('num_test', None)
    opts = MetricOptions(**kwargs)
    if num_test is not None:
        opts.num_test = num_test
    t0 = time.time()
    results = _metric_dict[metric](opts)
    total = time.time() - t0
    return EasyDict(results=EasyDict(results), metric=metric, total_time=total, total_time_str=f'{total:.1f}s', num_gpus=opts.num_gpus)


def report_metric(result_dict, run_dir=None, snapshot_pkl=None, alpha=None, num_steps_eval=None):
    """sid_metric_main.py:82-99: one JSON line on stdout and in `metric-<name>[-alpha-..][-num_steps_eval-..].jsonl`."""
    metric = result_dict['metric']
    if run_dir is not None and snapshot_pkl is not None:
        snapshot_pkl = os.path.relpath(snapshot_pkl, run_dir)
    line = json.dumps(dict(result_dict, snapshot_pkl=snapshot_pkl, timestamp=time.time()))
    dist.print0(line)
    if run_dir is not None and os.path.isdir(run_dir) and dist.get_rank() == 0:
        name = f'metric-{metric}'
        if alpha is not None:
            name += f'-alpha-{alpha:03f}'
            if num_steps_eval is not None and num_steps_eval != 1:
                name += f'-num_steps_eval-{num_steps_eval:02d}'
        with open(os.path.join(run_dir, name + '.jsonl'), 'at') as f:
            f.write(line + '\n')
    return line
