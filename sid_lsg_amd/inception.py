"""The Inception-v3 behind FID, KID, precision / recall and the Inception Score, on this package's HIP kernels.

The network is the FID variant pytorch-fid documents to match the 2015 TensorFlow graph (`pt_inception-2015-12-05`): torchvision's
Inception-v3 layout with 1008 output classes, the pooled branch of the A and C blocks and of Mixed_7b a 3 x 3 average that EXCLUDES
the padding, and Mixed_7c's pooled branch a 3 x 3 MAX pool.  That table is restated from the published description; it is not pinned
against the TorchScript file the reference downloads, which no machine without it can inspect (such a file keeps running through
torch.jit, metrics.load_detector).  What is pinned (tests/test_gpu_inception.py) is that this module computes that network: every
kernel against fp64, blocks and the whole chain against a plain torch.nn restatement in fp64.

How it runs (csrc/inception.hip, all fp32):
  * uint8 NCHW images -> one launch: TF's legacy bilinear resize to 299 x 299 (source coordinate i * W / 299 formed exactly in
    integers, `resize_plan`; what the detector's affine_grid / grid_sample pair computes) and (v - 128) / 128, NHWC with 4 channels;
  * all 94 convolutions through ops.conv2d_relu_f32 (implicit GEMM on the f32 MFMA) with the BatchNorm (eps 1e-3) folded into weight
    and bias once at load, in fp64, rounded to fp32 once (`fold_bn`); a branch writes its channel slice of the block's output, so no
    concat exists; pools through ops.pool2d_f32; fc through the fp32 GEMM in 8 slices of K whose partial logits are added in
    fp64 (`probabilities`); the softmax over 1008 logits is torch's, in fp64.
  * activations live in buffers kept per batch size; results are fresh tensors.  Forward only, under torch.no_grad.

Call contract of the TorchScript detector: det(uint8 NCHW, return_features=True) -> [B, 2048]; det(images) -> softmax [B, 1008];
det(images, no_output_bias=True) -> the same without fc's bias (what the Inception Score reads).

Weights: a torch.save'd state dict in torchvision / pytorch-fid key names (`load_state_dict_file`), or the seeded
'random:inception-v3[:seed]' (`random_state_dict`) for smoke runs and tests, whose scores mean nothing outside this package.
"""
import math
import os

import numpy as np
import torch

from . import distributed as dist
from . import ops

SIDE, FEATURES, CLASSES, BN_EPS = 299, 2048, 1008, 1e-3
RANDOM_PREFIX = 'random:inception-v3'
FC_SPLITS = 8             # K slices of the fc (HipInceptionV3.probabilities)
MAX_BATCH = 64            # images per pass: larger batches go through in chunks (the buffers of a pass are about 36 MB per image)


def _conv(name, cout, k=1, stride=1, pad=0):
    kh, kw = (k, k) if isinstance(k, int) else k
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    return ('conv', name, cout, kh, kw, stride, ph, pw)


def _pool(mode, k=3, stride=1, pad=0):
    return ('pool', mode, k, stride, pad)


def _fork(a, b):
    """The two convolutions that end a branch of the E blocks: both read the branch, their outputs sit side by side."""
    return ('fork', a, b)


def _block_a(pool_features):
    return [[_conv('branch1x1', 64)],
            [_conv('branch5x5_1', 48), _conv('branch5x5_2', 64, 5, pad=2)],
            [_conv('branch3x3dbl_1', 64), _conv('branch3x3dbl_2', 96, 3, pad=1), _conv('branch3x3dbl_3', 96, 3, pad=1)],
            [_pool(ops.POOL_MEAN, 3, 1, 1), _conv('branch_pool', pool_features)]]


def _block_b():
    return [[_conv('branch3x3', 384, 3, stride=2)],
            [_conv('branch3x3dbl_1', 64), _conv('branch3x3dbl_2', 96, 3, pad=1), _conv('branch3x3dbl_3', 96, 3, stride=2)],
            [_pool(ops.POOL_MAX, 3, 2)]]


def _block_c(c7):
    return [[_conv('branch1x1', 192)],
            [_conv('branch7x7_1', c7), _conv('branch7x7_2', c7, (1, 7), pad=(0, 3)), _conv('branch7x7_3', 192, (7, 1), pad=(3, 0))],
            [_conv('branch7x7dbl_1', c7), _conv('branch7x7dbl_2', c7, (7, 1), pad=(3, 0)), _conv('branch7x7dbl_3', c7, (1, 7), pad=(0, 3)),
             _conv('branch7x7dbl_4', c7, (7, 1), pad=(3, 0)), _conv('branch7x7dbl_5', 192, (1, 7), pad=(0, 3))],
            [_pool(ops.POOL_MEAN, 3, 1, 1), _conv('branch_pool', 192)]]


def _block_d():
    return [[_conv('branch3x3_1', 192), _conv('branch3x3_2', 320, 3, stride=2)],
            [_conv('branch7x7x3_1', 192), _conv('branch7x7x3_2', 192, (1, 7), pad=(0, 3)), _conv('branch7x7x3_3', 192, (7, 1), pad=(3, 0)),
             _conv('branch7x7x3_4', 192, 3, stride=2)],
            [_pool(ops.POOL_MAX, 3, 2)]]


def _block_e(pool_mode):
    return [[_conv('branch1x1', 320)],
            [_conv('branch3x3_1', 384), _fork(_conv('branch3x3_2a', 384, (1, 3), pad=(0, 1)), _conv('branch3x3_2b', 384, (3, 1), pad=(1, 0)))],
            [_conv('branch3x3dbl_1', 448), _conv('branch3x3dbl_2', 384, 3, pad=1),
             _fork(_conv('branch3x3dbl_3a', 384, (1, 3), pad=(0, 1)), _conv('branch3x3dbl_3b', 384, (3, 1), pad=(1, 0)))],
            [_pool(pool_mode, 3, 1, 1), _conv('branch_pool', 192)]]


# (name, step) for the stem, (name, [branch, ...]) for a block; the stem's pools carry no parameters and so no torchvision name
LAYERS = [
    ('Conv2d_1a_3x3', _conv('', 32, 3, stride=2)), ('Conv2d_2a_3x3', _conv('', 32, 3)), ('Conv2d_2b_3x3', _conv('', 64, 3, pad=1)),
    ('maxpool1', _pool(ops.POOL_MAX, 3, 2)), ('Conv2d_3b_1x1', _conv('', 80)), ('Conv2d_4a_3x3', _conv('', 192, 3)),
    ('maxpool2', _pool(ops.POOL_MAX, 3, 2)),
    ('Mixed_5b', _block_a(32)), ('Mixed_5c', _block_a(64)), ('Mixed_5d', _block_a(64)),
    ('Mixed_6a', _block_b()),
    ('Mixed_6b', _block_c(128)), ('Mixed_6c', _block_c(160)), ('Mixed_6d', _block_c(160)), ('Mixed_6e', _block_c(192)),
    ('Mixed_7a', _block_d()),
    ('Mixed_7b', _block_e(ops.POOL_MEAN)), ('Mixed_7c', _block_e(ops.POOL_MAX)),
]


def _step_convs(prefix, step, cin):
    """-> ([(key, cin, cout, kh, kw)], channels out) of one step."""
    if step[0] == 'pool':
        return [], cin
    if step[0] == 'fork':
        a, ca = _step_convs(prefix, step[1], cin)
        b, cb = _step_convs(prefix, step[2], cin)
        return a + b, ca + cb
    key = prefix + ('.' + step[1] if step[1] else '')
    return [(key, cin, step[2], step[3], step[4])], step[2]


def conv_table():
    """Every convolution of the network in execution order: [(torchvision module name, Cin, Cout, KH, KW)] (94 entries), and the
    input width of every layer of LAYERS: {layer name: Cin}."""
    table, widths, cin = [], {}, 3
    for name, spec in LAYERS:
        widths[name] = cin
        if isinstance(spec, list):
            total = 0
            for branch in spec:
                c = cin
                for step in branch:
                    t, c = _step_convs(name, step, c)
                    table += t
                total += c
            cin = total
        else:
            t, cin = _step_convs(name, spec, cin)
            table += t
    return table, widths


def expected_shapes():
    """{state-dict key: shape} of every tensor the loader reads."""
    shapes = {}
    for key, cin, cout, kh, kw in conv_table()[0]:
        shapes[key + '.conv.weight'] = (cout, cin, kh, kw)
        for p in ('weight', 'bias', 'running_mean', 'running_var'):
            shapes[f'{key}.bn.{p}'] = (cout,)
    shapes['fc.weight'] = (CLASSES, FEATURES)
    shapes['fc.bias'] = (CLASSES,)
    return shapes


def check_state_dict(sd):
    """The tensors of `sd` (optionally under 'state_dict') the network reads, checked by name: a missing key is a KeyError, a wrong
    shape a ValueError.  AuxLogits.* and num_batches_tracked are ignored, as is anything else the network does not read."""
    if isinstance(sd, dict) and isinstance(sd.get('state_dict'), dict):
        sd = sd['state_dict']
    if not isinstance(sd, dict):
        raise ValueError(f'Inception-v3 weights: expected a state dict, got {type(sd).__name__}')
    out = {}
    for key, shape in expected_shapes().items():
        if key not in sd:
            raise KeyError(f'Inception-v3 state dict: missing key {key!r}')
        t = torch.as_tensor(sd[key])
        if tuple(t.shape) != shape:
            raise ValueError(f'Inception-v3 state dict: {key!r} has shape {tuple(t.shape)}, expected {shape}')
        out[key] = t
    return out


def looks_like_state_dict(obj):
    """A mapping that claims to be this network's weights (so that a broken one is refused by name and not handed to torch.jit)."""
    if isinstance(obj, dict) and isinstance(obj.get('state_dict'), dict):
        obj = obj['state_dict']
    return isinstance(obj, dict) and any(isinstance(k, str) and (k.startswith('Conv2d_1a_3x3.') or k.startswith('Mixed_')) for k in obj)


def load_state_dict_file(path):
    """The state dict in `path`, or None when the file is not one: torch.load(weights_only=True) refuses TorchScript archives and
    pickled modules, which stay with metrics.load_detector's torch.jit / pickle chain."""
    import zipfile
    try:
        if zipfile.is_zipfile(path):
            with zipfile.ZipFile(path) as z:
                if any(n.endswith('/constants.pkl') for n in z.namelist()):      # a TorchScript archive: torch.load would hand it to torch.jit
                    return None
        obj = torch.load(path, map_location='cpu', weights_only=True)
    except Exception:
        return None
    return obj if looks_like_state_dict(obj) else None


def is_random_spec(path):
    return isinstance(path, str) and (path.lower() == RANDOM_PREFIX or path.lower().startswith(RANDOM_PREFIX + ':'))


def random_state_dict(seed=0):
    """Seeded weights that keep the 2048 features alive (mean 2.4, std 3.4, 13 % zeros on structured images): conv N(0, 2 / fan_in);
    BatchNorm weight U(0.5, 1.5), bias 0.1 N, running mean 0.1 N, running var U(0.5, 1.5); fc N(0, 1 / 2048), bias 0.1 N."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for key, cin, cout, kh, kw in conv_table()[0]:
        sd[key + '.conv.weight'] = torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(2.0 / (cin * kh * kw))
        sd[key + '.bn.weight'] = torch.rand(cout, generator=g) + 0.5
        sd[key + '.bn.bias'] = 0.1 * torch.randn(cout, generator=g)
        sd[key + '.bn.running_mean'] = 0.1 * torch.randn(cout, generator=g)
        sd[key + '.bn.running_var'] = torch.rand(cout, generator=g) + 0.5
    sd['fc.weight'] = torch.randn(CLASSES, FEATURES, generator=g) * math.sqrt(1.0 / FEATURES)
    sd['fc.bias'] = 0.1 * torch.randn(CLASSES, generator=g)
    return sd


def fold_bn(weight, gamma, beta, mean, var, eps=BN_EPS):
    """conv [Cout, Cin, KH, KW] followed by an eval-mode BatchNorm as one convolution: w' = w * gamma / sqrt(var + eps) and
    b' = beta - mean * gamma / sqrt(var + eps), evaluated in fp64 and rounded to fp32 once -> (w' [Cout, Cin, KH, KW], b' [Cout])."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return (weight.double() * s[:, None, None, None]).float(), (beta.double() - mean.double() * s).float()


def resize_plan(size, out=SIDE):
    """The taps of the legacy-TF bilinear resize of one axis, in integers: output i reads pixels q[i] = (i * size) // out and
    q1[i] = min(q[i] + 1, size - 1) with the weight rem[i] / out on the second, rem[i] = (i * size) % out.  -> (q, rem, q1) int64."""
    p = np.arange(out, dtype=np.int64) * int(size)
    q = p // out
    return q, p - q * out, np.minimum(q + 1, int(size) - 1)


_warned = set()


class HipInceptionV3:
    """FID's Inception-v3 from a state dict in torchvision / pytorch-fid key names; see the module docstring."""

    def __init__(self, state_dict, device='cuda', max_batch=MAX_BATCH, note=None):
        sd = check_state_dict(state_dict)
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        self.note = note
        self.widths = conv_table()[1]
        self.convs = {}
        for key, cin, cout, kh, kw in conv_table()[0]:
            w, b = fold_bn(sd[key + '.conv.weight'], sd[key + '.bn.weight'], sd[key + '.bn.bias'], sd[key + '.bn.running_mean'],
                           sd[key + '.bn.running_var'])
            w = w.permute(0, 2, 3, 1)                                      # [Cout, KH, KW, Cin]
            if cin % 4:                                                    # the stem: a zero weight for the zero plane
                w = torch.nn.functional.pad(w, [0, -cin % 4])
            self.convs[key] = (w.contiguous().to(self.device), b.contiguous().to(self.device))
        # fc as FC_SPLITS contiguous K slices [FC_SPLITS][1008][2048 / FC_SPLITS]: see probabilities()
        self.fc_weight = sd['fc.weight'].float().reshape(CLASSES, FC_SPLITS, FEATURES // FC_SPLITS).permute(1, 0, 2).contiguous().to(self.device)
        self.fc_bias = sd['fc.bias'].double().to(self.device)
        self._bufs = {}

    # ---- execution ----
    def _buf(self, key, shape):
        t = self._bufs.get((key,) + shape)
        if t is None:
            t = self._bufs[(key,) + shape] = torch.empty(shape, device=self.device, dtype=torch.float32)
        return t

    @staticmethod
    def _out_hw(step, h, w):
        if step[0] == 'fork':
            step = step[1]
        if step[0] == 'pool':
            _, _, k, s, p = step
            return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        _, _, _, kh, kw, s, ph, pw = step
        return (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1

    def _step(self, prefix, step, x, out=None, col=0):
        """One step on x [B, H, W, C] -> its output (a kept buffer, or columns of `out` from `col`) and the width it wrote."""
        B, H, W, _ = x.shape
        if step[0] == 'fork':
            _, wa = self._step(prefix, step[1], x, out, col)
            _, wb = self._step(prefix, step[2], x, out, col + wa)
            return out, wa + wb
        ho, wo = self._out_hw(step, H, W)
        if step[0] == 'pool':
            _, mode, k, s, p = step
            if out is None:
                out = self._buf(prefix + '.pool', (B, ho, wo, x.shape[3]))
            return ops.pool2d_f32(x, k, s, p, mode, out=out, col=col), x.shape[3]
        _, name, cout, kh, kw, s, ph, pw = step
        key = prefix + ('.' + name if name else '')
        w, b = self.convs[key]
        if out is None:
            out = self._buf(key, (B, ho, wo, cout))
        return ops.conv2d_relu_f32(x, w, b, stride=s, padding=(ph, pw), relu=True, out=out, col=col), cout

    def layer(self, name, x):
        """One entry of LAYERS on x [B, H, W, Cin] fp32 NHWC (the stem's first convolution: 4 channels) -> [B, Ho, Wo, Cout], a
        buffer this object keeps and overwrites on its next call at that shape."""
        spec = dict(LAYERS)[name]
        cin = self.widths[name]
        if x.dim() != 4 or x.shape[3] != cin + (-cin % 4) or x.dtype != torch.float32:
            raise ValueError(f'{name}: expected fp32 [B, H, W, {cin + (-cin % 4)}], got {x.dtype} {tuple(x.shape)}')
        if not isinstance(spec, list):
            return self._step(name, spec, x)[0]
        B, H, W, _ = x.shape
        ends, total = [], 0
        for branch in spec:
            h, w, c = H, W, cin
            for step in branch:
                h, w = self._out_hw(step, h, w)
                c = _step_convs(name, step, c)[1]
            ends.append((h, w))
            total += c
        if len(set(ends)) != 1:
            raise ValueError(f'{name}: the branches end at different sizes {ends} for a {H} x {W} input')
        out = self._buf(name, (B,) + ends[0] + (total,))
        col = 0
        for branch in spec:
            h = x
            for step in branch[:-1]:
                h = self._step(name, step, h)[0]
            col += self._step(name, branch[-1], h, out, col)[1]
        return out

    def features(self, images):
        """uint8 NCHW [B, 3, H, W] (B <= max_batch) -> [B, 2048] fp32, a fresh tensor."""
        B = images.shape[0]
        x = ops.inception_input_u8(images, out=self._buf('input', (B, SIDE, SIDE, 4)))
        for name, _ in LAYERS:
            x = self.layer(name, x)
        if x.shape[1:] != (8, 8, FEATURES):
            raise RuntimeError(f'Inception-v3: the last block gave {tuple(x.shape)}')
        return ops.pool2d_f32(x, 8, 8, 0, ops.POOL_MEAN).reshape(B, FEATURES)

    def probabilities(self, features, no_output_bias=False):
        """[B, 2048] features -> softmax over the 1008 logits, fp32.  One fp32 fma chain over all 2048 features carries partial sums
        of the size of the largest logit (10 - 20) through 2048 roundings: about 3e-6 on a logit and 2e-6 on a probability near 1/2.
        So the fc runs as FC_SPLITS fp32 GEMMs over K slices of 256, and their partial logits (and the bias) are added, and the
        softmax taken, in fp64: what is left is the error of the features."""
        B, step = features.shape[0], FEATURES // FC_SPLITS
        parts = self._buf('fc', (FC_SPLITS, B, CLASSES))
        for i in range(FC_SPLITS):
            ops.gemm(features[:, i * step:(i + 1) * step], self.fc_weight[i], out=parts[i])
        logits = parts.double().sum(0)
        if not no_output_bias:
            logits = logits + self.fc_bias
        return torch.softmax(logits, dim=1).float()

    @torch.no_grad()
    def __call__(self, images, return_features=False, no_output_bias=False):
        if self.note and self.note not in _warned:
            _warned.add(self.note)
            dist.print0(self.note)
        images = torch.as_tensor(images)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f'HipInceptionV3: expected uint8 NCHW images with 3 channels, got {images.dtype} {tuple(images.shape)}')
        images = images.to(self.device).contiguous()
        outs = []
        for i in range(0, images.shape[0], self.max_batch):
            f = self.features(images[i:i + self.max_batch])
            if not return_features:
                f = self.probabilities(f, no_output_bias)
            outs.append(f)
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


def load_inception(path, device):
    """'random:inception-v3[:seed]' or a state-dict file -> HipInceptionV3."""
    if is_random_spec(path):
        seed = path[len(RANDOM_PREFIX) + 1:] or '0'
        if not seed.isdigit():
            raise ValueError(f'{path!r}: expected {RANDOM_PREFIX}[:seed] with an integer seed')
        note = (f'NOTE: {path}: seeded random Inception-v3 weights -- FID / KID / precision / recall / IS from it are not comparable with '
                'published scores')
        return HipInceptionV3(random_state_dict(int(seed)), device, note=note)
    sd = load_state_dict_file(path)
    if sd is None:
        raise ValueError(f'{os.fspath(path)!r} is not an Inception-v3 state dict (torch.save of torchvision / pytorch-fid key names)')
    return HipInceptionV3(sd, device)
