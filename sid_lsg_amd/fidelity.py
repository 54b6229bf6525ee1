"""Paired image fidelity: PSNR, SSIM and LPIPS of an image against the image it started from, on this package's HIP kernels.

FID, KID, CMMD, IS, precision / recall, CLIP score and HPSv2 score a set of images or an image against a prompt.  The edit paths
(--init_images, --mask_images, --controlnet, --ip_adapter) need the other question: how much of the init image is left.

`psnr_ssim` (sidlsg_psnr_ssim_u8, csrc/fidelity.hip): one pass over two uint8 NCHW image sets.  The squared error is an exact integer;
SSIM is Wang et al.'s index with the 11 x 11 Gaussian window (sigma 1.5), K1 = 0.01, K2 = 0.03, L = 255, population moments, valid
windows only, averaged over the three channels, with the moments and the formula in fp64.  With a mask (uint8 [B, H, W], kept = < 128,
the convention of --mask_images) the `_keep` figures restrict the squared error to kept pixels and SSIM to windows whose CENTRE pixel is
kept.

`HipLPIPS`: LPIPS with the VGG16 backbone, forward only, all fp32.  The rules are restated from the source of the published `lpips`
package (v0.1: the scaling layer's shift and scale, the five taps after relu1_2 .. relu5_3, unit-normalised features with eps 1e-10
added to the norm, the non-negative 1 x 1 `lin` weights, the spatial mean, the sum over taps); they are not pinned against that
package, which no machine without it can run.  What is pinned (tests/test_gpu_fidelity.py) is that this module computes those rules:
each kernel against fp64, the whole chain against a torch.nn restatement in fp64.  Both image sets travel as ONE batch of 2B from the
input launch on (sidlsg_lpips_input_u8), the 13 convolutions run on ops.conv2d_relu_f32, the four pools on ops.pool2d_f32, each tap is
one sidlsg_lpips_layer_f32 launch, and the five per-tap values of a pair are added in tap order by one more (sidlsg_lpips_sum_f64).  LPIPS-Alex is not offered: its 11 x 11 /
stride 4 first layer is outside the convolution's admitted set.

`HipLPIPS.group_pairs` is the all-pairs form behind sid_lsg_amd.diversity: VGG16 once per image (`features`), and every tap one
sidlsg_lpips_group_f32 launch that forms the K (K - 1) / 2 pairs of a group of K maps in place, each value the bits the paired launch
gives that pair.

Weights: a torch.save'd VGG16 state dict in torchvision key names and the lpips package's lin weights, or the seeded
'random:lpips-vgg[:seed]' for both, whose scores mean nothing outside this package.
"""
import math
import os

import torch

from . import distributed as dist
from . import ops
from ._lib import lib

RANDOM_PREFIX = 'random:lpips-vgg'
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# torchvision's vgg16.features: (index, Cin, Cout) of the 13 convolutions, 'M' = the 2 x 2 / stride 2 max pool, 'T' = a tap
VGG_LAYERS = [(0, 3, 64), (2, 64, 64), 'T', 'M', (5, 64, 128), (7, 128, 128), 'T', 'M', (10, 128, 256), (12, 256, 256), (14, 256, 256), 'T', 'M',
              (17, 256, 512), (19, 512, 512), (21, 512, 512), 'T', 'M', (24, 512, 512), (26, 512, 512), (28, 512, 512), 'T']
TAP_CHANNELS = (64, 128, 256, 512, 512)
LIMIT = 1 << 31           # an operand of a kernel stays below this many bytes
KEYS = ('mse', 'psnr', 'ssim')
KEEP_KEYS = ('mse_keep', 'psnr_keep', 'ssim_keep')


# ---- PSNR / SSIM ----
def _psnr(mse):
    if mse != mse:
        return float('nan')
    return float('inf') if mse == 0 else 10.0 * math.log10(65025.0 / mse)


def _check_pair(name, a, b):
    for t, n in ((a, 'a'), (b, 'b')):
        ops._chk(t, torch.uint8)
        if t.dim() != 4 or t.shape[1] != 3:
            raise RuntimeError(f'{name}: {n}: expected uint8 [B, 3, H, W], got {tuple(t.shape)}')
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f'{name}: a {tuple(a.shape)} on {a.device} and b {tuple(b.shape)} on {b.device}: one shape, one device')


def psnr_ssim_sums(a, b, mask=None):
    """uint8 [B, 3, H, W] a and b (mask: uint8 [B, H, W], kept = < 128; None = all kept) -> [B, 8] fp64 on the device:
    sse, n, ssim_sum, ssim_n, and the same four over kept positions (sidlsg_psnr_ssim_u8)."""
    _check_pair('psnr_ssim', a, b)
    B, _, H, W = a.shape
    if mask is not None:
        ops._chk(mask, torch.uint8)
        if tuple(mask.shape) != (B, H, W) or mask.device != a.device:
            raise RuntimeError(f'psnr_ssim: mask {tuple(mask.shape)} on {mask.device}: expected uint8 [{B}, {H}, {W}] on {a.device}')
    nws = lib.sidlsg_psnr_ssim_ws_doubles.raw(B, H, W)
    if nws < 0:
        raise RuntimeError(f'psnr_ssim: {B} images of {H} x {W}: need H, W >= 11, 1 <= B <= 21845 and fewer than 2^31 bytes per operand')
    ws = torch.empty(nws, device=a.device, dtype=torch.float64)
    out = torch.empty((B, 8), device=a.device, dtype=torch.float64)
    lib.sidlsg_psnr_ssim_u8(ops._p(a), ops._p(b), ops._p(mask), B, H, W, ops._p(out), ops._p(ws), ops._s())
    return out


def metrics_from_sums(sums, with_keep):
    """[B][8] (psnr_ssim_sums, on the host) -> one dict per image: mse, psnr = 10 log10(65025 / mse) (inf at mse == 0), ssim, and with
    `with_keep` the three `_keep` figures (nan for an image with no kept term)."""
    rows = []
    for sse, n, ss, sn, sse_k, n_k, ss_k, sn_k in sums:
        mse = sse / n
        row = {'mse': mse, 'psnr': _psnr(mse), 'ssim': ss / sn}
        if with_keep:
            mse_k = sse_k / n_k if n_k > 0 else float('nan')
            row.update(mse_keep=mse_k, psnr_keep=_psnr(mse_k), ssim_keep=ss_k / sn_k if sn_k > 0 else float('nan'))
        rows.append(row)
    return rows


def psnr_ssim(a_u8, b_u8, mask=None):
    """-> one dict per image: mse, psnr, ssim; with a mask also mse_keep, psnr_keep, ssim_keep."""
    return metrics_from_sums(psnr_ssim_sums(a_u8, b_u8, mask).cpu().tolist(), mask is not None)


def aggregate(per_image):
    """The figures of a set from its per-image dicts (a list, or a dict keyed by file name): ssim, mse and lpips are the means of the
    per-image values; psnr is computed FROM THE MEAN MSE, so one bit-identical pair (psnr inf) does not make the set's figure infinite.
    The `_keep` keys likewise, over the images that have kept terms (nan when none has)."""
    rows = list(per_image.values()) if isinstance(per_image, dict) else list(per_image)
    if not rows:
        raise ValueError('aggregate: no images')

    def mean(key):
        vals = [r[key] for r in rows if key in r and r[key] == r[key]]
        return sum(vals) / len(vals) if vals else float('nan')
    out = {'mse': mean('mse'), 'ssim': mean('ssim')}
    out['psnr'] = _psnr(out['mse'])
    if any('mse_keep' in r for r in rows):
        out['mse_keep'], out['ssim_keep'] = mean('mse_keep'), mean('ssim_keep')
        out['psnr_keep'] = _psnr(out['mse_keep'])
    if any('lpips' in r for r in rows):
        out['lpips'] = mean('lpips')
    return out


# ---- LPIPS ----
def lpips_input_u8(a, b, out=None):
    """uint8 [B, 3, H, W] a and b -> fp32 NHWC [2B, H, W, 4] (sidlsg_lpips_input_u8): rows 0 .. B-1 from a, B .. 2B-1 from b,
    (x / 127.5 - 1 - shift_c) / scale_c rounded operation by operation, channel 3 zero."""
    _check_pair('lpips_input_u8', a, b)
    B, _, H, W = a.shape
    if out is None:
        out = torch.empty((2 * B, H, W, 4), device=a.device, dtype=torch.float32)
    ops._chk(out, torch.float32)
    if tuple(out.shape) != (2 * B, H, W, 4):
        raise RuntimeError(f'lpips_input_u8: out {tuple(out.shape)}, expected {(2 * B, H, W, 4)}')
    lib.sidlsg_lpips_input_u8(ops._p(a), ops._p(b), ops._p(out), B, H, W, *SHIFT, *SCALE, ops._s())
    return out


def lpips_layer_f32(feats, w, out=None):
    """feats fp32 NHWC [2B, h, wd, ldf], w [C] (C <= ldf) -> [B] fp64 (sidlsg_lpips_layer_f32): the spatial mean of the lin-weighted
    squared difference of the unit-normalised features of rows i and B + i."""
    ops._chk(feats, torch.float32), ops._chk(w, torch.float32)
    if feats.dim() != 4 or feats.shape[0] % 2 or w.dim() != 1 or w.shape[0] > feats.shape[3]:
        raise RuntimeError(f'lpips_layer_f32: feats {tuple(feats.shape)}, w {tuple(w.shape)}')
    B2, h, wd, ldf = feats.shape
    B = B2 // 2
    nws = lib.sidlsg_lpips_layer_ws_doubles.raw(B, h, wd)
    if nws < 0:
        raise RuntimeError(f'lpips_layer_f32: {B} pairs of {h} x {wd} pixels are outside the admitted set')
    if out is None:
        out = torch.empty(B, device=feats.device, dtype=torch.float64)
    ws = torch.empty(nws, device=feats.device, dtype=torch.float64)
    lib.sidlsg_lpips_layer_f32(ops._p(feats), ldf, ops._p(w), B, h, wd, w.shape[0], ops._p(out), ops._p(ws), ops._s())
    return out


GROUP_MAX = 16            # images per group that sidlsg_lpips_group_f32 admits


GROUP_FORMS = {None: 0, 'chip': 1, 'pairs': 2}


def lpips_group_f32(feats, w, K, out=None, form=None):
    """feats fp32 NHWC [G*K, h, wd, ldf], w [C] (C <= ldf) -> [G, K (K - 1) / 2] fp64 (sidlsg_lpips_group_f32): what lpips_layer_f32
    gives for every pair (i, j), i < j, of the K rows of a group, in lexicographic pair order, bit for bit.  `form` names the launch
    form for tests and measurements ('chip': all pairs of a pixel block in one workgroup; 'pairs': one workgroup per block and pair);
    None lets the library choose by the size of the map.  The forms write the same bits."""
    ops._chk(feats, torch.float32), ops._chk(w, torch.float32)
    if feats.dim() != 4 or K < 2 or feats.shape[0] % K or w.dim() != 1 or w.shape[0] > feats.shape[3]:
        raise RuntimeError(f'lpips_group_f32: feats {tuple(feats.shape)}, w {tuple(w.shape)}, groups of {K}')
    N, h, wd, ldf = feats.shape
    G, P = N // K, K * (K - 1) // 2
    nws = lib.sidlsg_lpips_group_ws_doubles.raw(G, K, h, wd)
    if nws < 0:
        raise RuntimeError(f'lpips_group_f32: {G} groups of {K} maps of {h} x {wd} pixels are outside the admitted set (2 <= K <= {GROUP_MAX}, '
                           'at most 32767 maps and 32767 pairs)')
    if out is None:
        out = torch.empty((G, P), device=feats.device, dtype=torch.float64)
    ops._chk(out, torch.float64)
    if out.numel() != G * P:
        raise RuntimeError(f'lpips_group_f32: out {tuple(out.shape)}, expected {(G, P)}')
    ws = torch.empty(nws, device=feats.device, dtype=torch.float64)
    if form is None:
        lib.sidlsg_lpips_group_f32(ops._p(feats), ldf, ops._p(w), G, K, h, wd, w.shape[0], ops._p(out), ops._p(ws), ops._s())
    else:
        lib.sidlsg_lpips_group_form_f32(ops._p(feats), ldf, ops._p(w), G, K, h, wd, w.shape[0], GROUP_FORMS[form], ops._p(out), ops._p(ws), ops._s())
    return out


def vgg_shapes():
    """{state-dict key: shape} of the VGG16 tensors the network reads."""
    shapes = {}
    for step in VGG_LAYERS:
        if isinstance(step, tuple):
            i, cin, cout = step
            shapes[f'features.{i}.weight'] = (cout, cin, 3, 3)
            shapes[f'features.{i}.bias'] = (cout,)
    return shapes


def lin_shapes():
    return {f'lin{i}.model.1.weight': (1, c, 1, 1) for i, c in enumerate(TAP_CHANNELS)}


def _check(sd, shapes, what):
    if isinstance(sd, dict) and isinstance(sd.get('state_dict'), dict):
        sd = sd['state_dict']
    if not isinstance(sd, dict):
        raise ValueError(f'{what}: expected a state dict, got {type(sd).__name__}')
    out = {}
    for key, shape in shapes.items():
        if key not in sd:
            foreign = sorted(k for k in sd if isinstance(k, str))[:3]
            raise KeyError(f'{what}: missing key {key!r}' + (f' (the file holds {", ".join(map(repr, foreign))}, ...)' if foreign else ''))
        t = torch.as_tensor(sd[key])
        if tuple(t.shape) != shape:
            raise ValueError(f'{what}: {key!r} has shape {tuple(t.shape)}, expected {shape}')
        out[key] = t
    return out


def check_vgg_state_dict(sd):
    """The 26 `features.*` tensors of a torchvision VGG16 state dict, checked by name: a missing key is a KeyError, a wrong shape a
    ValueError.  Classifier keys, and anything else the network does not read, are ignored."""
    return _check(sd, vgg_shapes(), 'LPIPS VGG16 state dict')


def check_lin_state_dict(sd):
    """The five `lin{i}.model.1.weight` tensors of the lpips package's vgg.pth, checked by name."""
    return _check(sd, lin_shapes(), 'LPIPS lin state dict')


def is_random_spec(spec):
    return isinstance(spec, str) and (spec.lower() == RANDOM_PREFIX or spec.lower().startswith(RANDOM_PREFIX + ':'))


def random_state_dicts(seed=0):
    """Seeded (vgg, lin) state dicts: convolutions N(0, 2 / fan_in) (He: the features stay alive through 13 layers), biases 0.05 N,
    lin weights U(0, 2 / C) (non-negative, as the package's are)."""
    g = torch.Generator().manual_seed(int(seed))
    vgg, lin = {}, {}
    for key, shape in vgg_shapes().items():
        if key.endswith('.weight'):
            vgg[key] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * 9))
        else:
            vgg[key] = 0.05 * torch.randn(shape, generator=g)
    for key, shape in lin_shapes().items():
        lin[key] = torch.rand(shape, generator=g) * (2.0 / shape[1])
    return vgg, lin


_warned = set()


class HipLPIPS:
    """LPIPS-VGG from a torchvision VGG16 state dict and the lpips package's lin weights; see the module docstring.
    lp(a_u8, b_u8) -> [B] fp64 on the device, one distance per pair."""

    def __init__(self, vgg_state_dict, lin_state_dict, device='cuda', note=None):
        vgg, lin = check_vgg_state_dict(vgg_state_dict), check_lin_state_dict(lin_state_dict)
        self.device = torch.device(device)
        self.note = note
        self.convs = {}
        for step in VGG_LAYERS:
            if isinstance(step, tuple):
                i, cin, _ = step
                w = vgg[f'features.{i}.weight'].float().permute(0, 2, 3, 1)          # [Cout, 3, 3, Cin]
                if cin % 4:                                                           # the first convolution: a zero weight for the zero plane
                    w = torch.nn.functional.pad(w, [0, -cin % 4])
                self.convs[i] = (w.contiguous().to(self.device), vgg[f'features.{i}.bias'].float().contiguous().to(self.device))
        self.lins = [lin[f'lin{i}.model.1.weight'].float().reshape(-1).contiguous().to(self.device) for i in range(len(TAP_CHANNELS))]
        self._bufs = {}

    def _buf(self, key, shape, dtype=torch.float32):
        t = self._bufs.get((key,) + shape)
        if t is None:
            t = self._bufs[(key,) + shape] = torch.empty(shape, device=self.device, dtype=dtype)
        return t

    @staticmethod
    def max_pairs(H, W):
        """Pairs per pass: the largest operand is the first stage's map, 2B x H x W x 64 fp32 (67 MB per image at 512 x 512).  It is
        kept to 2^30 bytes, half of what a kernel admits, which also bounds the buffers of a pass: 8 pairs at 512 x 512."""
        return (LIMIT // 2) // (2 * H * W * 64 * 4)

    def taps(self, a, b):
        """uint8 [B, 3, H, W] a and b -> the five tap feature maps [2B, h, w, C] (buffers this object keeps and overwrites)."""
        B, _, H, W = a.shape
        x = lpips_input_u8(a, b, out=self._buf('input', (2 * B, H, W, 4)))
        out, npool = [], 0
        for step in VGG_LAYERS:
            if step == 'T':
                out.append(x)
            elif step == 'M':
                if x.shape[1] < 2 or x.shape[2] < 2:
                    raise ValueError(f'LPIPS: {H} x {W} images are too small for the four 2 x 2 pools of VGG16 (at least 16 x 16)')
                npool += 1
                x = ops.pool2d_f32(x, 2, 2, 0, ops.POOL_MAX, out=self._buf(f'pool{npool}', (2 * B, x.shape[1] // 2, x.shape[2] // 2, x.shape[3])))
            else:
                w, bias = self.convs[step[0]]
                x = ops.conv2d_relu_f32(x, w, bias, stride=1, padding=(1, 1), relu=True, out=self._buf(f'conv{step[0]}', tuple(x.shape[:3]) + (step[2],)))
        return out

    def tap_values(self, a, b):
        """One pass (B <= max_pairs(H, W)): [5, B] fp64, the distance of every pair at every tap (a kept buffer)."""
        vals = self._buf('vals', (len(TAP_CHANNELS), a.shape[0]), torch.float64)
        for i, f in enumerate(self.taps(a, b)):
            lpips_layer_f32(f, self.lins[i], out=vals[i])
        return vals

    def pairs(self, a, b):
        """One pass: [B] fp64, a fresh tensor: the five per-tap values of a pair added in tap order (sidlsg_lpips_sum_f64)."""
        vals = self.tap_values(a, b)
        out = torch.empty(a.shape[0], device=self.device, dtype=torch.float64)
        lib.sidlsg_lpips_sum_f64(ops._p(vals), vals.shape[0], vals.shape[1], ops._p(out), ops._s())
        return out

    def features(self, images):
        """uint8 [N, 3, H, W] -> the five tap feature maps [N, h, w, C] of the N images (views of buffers this object keeps and
        overwrites).  The images travel as the two halves of one `taps` batch, an odd N padded by its last image, so an image's maps
        are the bits `taps` gives it."""
        N = images.shape[0]
        half = (N + 1) // 2
        b = images[half:] if N % 2 == 0 else torch.cat([images[half:], images[-1:]])
        return [f[:N] for f in self.taps(images[:half], b)]

    def group_pass(self, images, K):
        """One pass (at most 2 max_pairs(H, W) images, whole groups): [G, K (K - 1) / 2] fp64, a fresh tensor.  1 input + 13 convolution
        + 4 pool + 5 group-layer + 1 sum launches, whatever K is."""
        G, P = images.shape[0] // K, K * (K - 1) // 2
        vals = self._buf('gvals', (len(TAP_CHANNELS), G * P), torch.float64)
        for i, f in enumerate(self.features(images)):
            lpips_group_f32(f, self.lins[i], K, out=vals[i])
        out = torch.empty((G, P), device=self.device, dtype=torch.float64)
        lib.sidlsg_lpips_sum_f64(ops._p(vals), vals.shape[0], vals.shape[1], ops._p(out), ops._s())
        return out

    @torch.no_grad()
    def group_pairs(self, images, K):
        """uint8 [G*K, 3, H, W], group g = images gK .. gK+K-1 -> [G, K (K - 1) / 2] fp64: LPIPS of every pair (i, j), i < j, of a
        group in lexicographic pair order, each entry the bits of self(a_i[None], a_j[None]).  VGG16 runs once per image."""
        if self.note and self.note not in _warned:
            _warned.add(self.note)
            dist.print0(self.note)
        images = torch.as_tensor(images).to(self.device).contiguous()
        ops._chk(images, torch.uint8)
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
            raise RuntimeError(f'HipLPIPS.group_pairs: expected uint8 [G*K, 3, H, W], got {tuple(images.shape)}')
        N, _, H, W = images.shape
        if not 2 <= K <= GROUP_MAX or N % K:
            raise ValueError(f'HipLPIPS.group_pairs: {N} images in groups of {K}: expected 2 <= K <= {GROUP_MAX} and whole groups')
        per_pass = 2 * self.max_pairs(H, W)
        if K > per_pass:
            raise ValueError(f'HipLPIPS.group_pairs: a group of K = {K} images of {H} x {W} exceeds one pass ({per_pass} images: the first '
                             "stage's map is kept to 2^30 bytes)")
        groups = max(1, min(per_pass // K, 32767 // (K * (K - 1) // 2)))
        outs = [self.group_pass(images[g * K:(g + groups) * K], K) for g in range(0, N // K, groups)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    @torch.no_grad()
    def __call__(self, a, b):
        if self.note and self.note not in _warned:
            _warned.add(self.note)
            dist.print0(self.note)
        a, b = torch.as_tensor(a).to(self.device).contiguous(), torch.as_tensor(b).to(self.device).contiguous()
        _check_pair('HipLPIPS', a, b)
        step = self.max_pairs(a.shape[2], a.shape[3])
        if step < 1:
            raise ValueError(f'LPIPS: one pair of {a.shape[2]} x {a.shape[3]} images exceeds 2^31 bytes in the first stage')
        outs = [self.pairs(a[i:i + step], b[i:i + step]) for i in range(0, a.shape[0], step)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)


def _load_file(path, what):
    if not os.path.isfile(path):
        raise ValueError(f'{what} {os.fspath(path)!r}: not a file (a torch.save\'d state dict, or {RANDOM_PREFIX}[:seed])')
    try:
        return torch.load(path, map_location='cpu', weights_only=True)
    except Exception as e:
        raise ValueError(f'{what} {os.fspath(path)!r}: not a torch.save\'d state dict ({type(e).__name__})')


def check_specs(vgg_spec, lin_spec):
    """Both given, and both random or both files: refused by name otherwise (before any weight is read)."""
    if not vgg_spec or not lin_spec:
        raise ValueError('LPIPS needs both --lpips_vgg (a torchvision VGG16 state dict) and --lpips_lin (the lpips package\'s vgg.pth), '
                         f'or {RANDOM_PREFIX}[:seed] for both')
    if is_random_spec(vgg_spec) != is_random_spec(lin_spec) or (is_random_spec(vgg_spec) and vgg_spec.lower() != lin_spec.lower()):
        raise ValueError(f'--lpips_vgg {vgg_spec!r} and --lpips_lin {lin_spec!r}: {RANDOM_PREFIX}[:seed] is given for both, with one seed, or for neither')
    if is_random_spec(vgg_spec):
        seed = vgg_spec[len(RANDOM_PREFIX) + 1:] or '0'
        if not seed.isdigit():
            raise ValueError(f'{vgg_spec!r}: expected {RANDOM_PREFIX}[:seed] with an integer seed')


def load_lpips(vgg_spec, lin_spec, device):
    """'random:lpips-vgg[:seed]' for both, or two state-dict files -> HipLPIPS."""
    check_specs(vgg_spec, lin_spec)
    if is_random_spec(vgg_spec):
        seed = vgg_spec[len(RANDOM_PREFIX) + 1:] or '0'
        note = f'NOTE: {vgg_spec}: seeded random LPIPS-VGG weights -- LPIPS from them is not comparable with published scores'
        return HipLPIPS(*random_state_dicts(int(seed)), device, note=note)
    return HipLPIPS(_load_file(vgg_spec, '--lpips_vgg'), _load_file(lin_spec, '--lpips_lin'), device)


# ---- scoring of a batch, shared by generate_onestep.py --fidelity and tools/image_pair_fidelity.py ----
def score_batch(ref_u8, test_u8, mask=None, lpips=None):
    """uint8 [B, 3, H, W] reference and test images on the device (mask: uint8 [B, H, W]) -> one dict per image."""
    rows = psnr_ssim(test_u8, ref_u8, mask)
    if lpips is not None:
        for row, v in zip(rows, lpips(test_u8, ref_u8).cpu().tolist()):
            row['lpips'] = v
    return rows


def format_means(mean):
    order = [k for k in KEYS + KEEP_KEYS + ('lpips',) if k in mean]
    return ', '.join(f'{k} {mean[k]:.6g}' for k in order)
