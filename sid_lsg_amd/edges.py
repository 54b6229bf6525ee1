"""Canny edge maps on the device, and edge adherence: does an output follow the edges it was conditioned on (csrc/canny.hip).

`canny(images)` is ControlNet's Canny annotator: OpenCV's `Canny(img, 100, 200)` (aperture 3, L1 gradient) restated rule by rule in
include/sidlsg_hip.h -- per-channel 3 x 3 Sobel with a replicated border, the channel of the largest |dx| + |dy|, non-maximum suppression
in integer arithmetic (TG22 = 13573), two thresholds, 8-connected hysteresis.  Two launches: sidlsg_canny_classify_u8 (a tile with a halo
of 2 in LDS, the candidate and strong planes written from wave64 ballots) and sidlsg_edge_hysteresis (one workgroup per image, both planes
in LDS, bit-parallel rounds until a workgroup-wide OR says nothing changed).  OpenCV is not a dependency; what the tests pin is an
independent numpy / scipy restatement of the same rules (tests/canny_ref.py), to the bit.

Edge maps travel as bit planes (`EdgeMaps.bits`: int32 [B, H, ceil(W / 32)], pixel x = bit x % 32 of word x // 32, padding bits zero).
`pack(images)` turns a control image, ours or a user's, into one (any channel >= 128).  `match(a, b, r)` counts per image |a|, |b|,
|a & D_r(b)| and |b & D_r(a)|, D_r the r-fold 3 x 3 dilation clipped to the image; `adherence_rows` / `aggregate` turn the counts of
(control, output) pairs into precision, recall and F1 with a pixel tolerance, the accepted measure for edge conditioning.
"""
import numpy as np
import torch

from . import ops
from ._lib import lib

HYST_LDS_MAX = 147456     # bytes of LDS sidlsg_edge_hysteresis admits for the two planes of an image: 768 x 768
MAX_TOLERANCE = 16
COUNT_KEYS = ('control_edges', 'output_edges', 'output_hits', 'control_hits')


def hysteresis_lds_bytes(H, W):
    """Bytes of LDS the two bit planes of an H x W image take (no device needed)."""
    return 2 * int(H) * ((int(W) + 31) // 32) * 4


def check_size(H, W, what='canny'):
    if hysteresis_lds_bytes(H, W) > HYST_LDS_MAX:
        raise ValueError(f'{what}: the two bit planes of a {H} x {W} image take {hysteresis_lds_bytes(H, W)} bytes, above the limit of '
                         f'{HYST_LDS_MAX} bytes of LDS the hysteresis keeps per image (768 x 768); larger images are not supported')


def check_thresholds(low, high):
    """ValueError naming the argument for anything the C side refuses."""
    for name, v in (('low', low), ('high', high)):
        if int(v) != v:
            raise ValueError(f'canny: {name} = {v!r}: the thresholds are integers')
        if v < 0:
            raise ValueError(f'canny: {name} = {v}: a threshold cannot be negative')
    if low > high:
        raise ValueError(f'canny: low = {low} is above high = {high}')


def check_tolerance(tolerance):
    if int(tolerance) != tolerance or not 0 <= tolerance <= MAX_TOLERANCE:
        raise ValueError(f'match: tolerance = {tolerance!r}: expected an integer in 0 .. {MAX_TOLERANCE}')


def _images(name, images):
    if not isinstance(images, torch.Tensor):
        images = torch.as_tensor(np.ascontiguousarray(images))
    if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8 or 0 in images.shape:
        raise ValueError(f'{name}: images: expected uint8 [B, H, W, 3] with B, H, W >= 1, got {images.dtype} {tuple(images.shape)}')
    if images.numel() >= 1 << 31:
        raise ValueError(f'{name}: images: {tuple(images.shape)} is 2^31 bytes or more')
    return ops._chk(images.contiguous(), torch.uint8)


class EdgeMaps:
    """B edge sets as bit planes.  bits: int32 [B, H, ceil(W / 32)] on the device; rounds: int32 [B], the hysteresis rounds of `canny`
    (None for a packed map)."""

    def __init__(self, bits, H, W, rounds=None, rgb=None):
        if bits.dtype != torch.int32 or bits.dim() != 3 or tuple(bits.shape[1:]) != (H, (W + 31) // 32):
            raise ValueError(f'EdgeMaps: bits: expected int32 [B, {H}, {(W + 31) // 32}] for {H} x {W} images, got {bits.dtype} {tuple(bits.shape)}')
        self.bits, self.H, self.W, self.rounds, self._rgb = bits, int(H), int(W), rounds, rgb

    @property
    def B(self):
        return self.bits.shape[0]

    def rgb_u8(self):
        """uint8 [B, H, W, 3] on the device: 255 in all three channels on an edge, 0 elsewhere (the control image a ControlNet takes)."""
        if self._rgb is None:
            self._rgb = hysteresis(self.bits, self.bits, self.H, self.W, want_edges=False, want_rgb=True)[1]      # E = hysteresis(E, E)
        return self._rgb

    def to_bool(self):
        """bool numpy [B, H, W] on the host."""
        return unpack_bits(self.bits.cpu().numpy(), self.W)


def unpack_bits(words, W):
    """int32 / uint32 [.., Wd] words -> bool [.., W] (host)."""
    w = np.ascontiguousarray(words).view(np.uint32)
    bits = (w[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(w.shape[:-1] + (-1,))[..., :W].astype(bool)


def pack_bits(mask):
    """bool [.., W] -> int32 [.., ceil(W / 32)] words (host), padding bits zero."""
    mask = np.asarray(mask, dtype=bool)
    W = mask.shape[-1]
    pad = np.zeros(mask.shape[:-1] + ((-W) % 32,), dtype=bool)
    m = np.concatenate([mask, pad], axis=-1).reshape(mask.shape[:-1] + (-1, 32))
    return (m.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).view(np.int32)


def _planes(name, arg, t, B, H, W):
    ops._chk(t, torch.int32)
    if tuple(t.shape) != (B, H, (W + 31) // 32):
        raise ValueError(f'{name}: {arg}: expected int32 {(B, H, (W + 31) // 32)} bit planes of {H} x {W} images, got {tuple(t.shape)}')
    return t


def classify(images, low=100, high=200):
    """uint8 [B, H, W, 3] -> (cand, strong) bit planes, int32 [B, H, Wd] (sidlsg_canny_classify_u8)."""
    check_thresholds(low, high)
    images = _images('classify', images)
    B, H, W, _ = images.shape
    cand = torch.empty((B, H, (W + 31) // 32), device=images.device, dtype=torch.int32)
    strong = torch.empty_like(cand)
    lib.sidlsg_canny_classify_u8(ops._p(images), ops._p(cand), ops._p(strong), B, H, W, int(low), int(high), ops._s())
    return cand, strong


def hysteresis(cand, strong, H, W, want_edges=True, want_rgb=False):
    """(cand, strong) planes -> (edges plane or None, uint8 [B, H, W, 3] or None, rounds int32 [B]) (sidlsg_edge_hysteresis)."""
    if cand.dim() != 3:
        raise ValueError(f'hysteresis: cand: expected int32 [B, H, Wd], got {tuple(cand.shape)}')
    B = cand.shape[0]
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f'hysteresis: B, H, W = {B}, {H}, {W}: all must be at least 1')
    _planes('hysteresis', 'cand', cand, B, H, W), _planes('hysteresis', 'strong', strong, B, H, W)
    check_size(H, W, 'hysteresis')
    if not (want_edges or want_rgb):
        raise ValueError('hysteresis: want_edges / want_rgb: at least one output')
    edges = torch.empty_like(cand) if want_edges else None
    rgb = torch.empty((B, H, W, 3), device=cand.device, dtype=torch.uint8) if want_rgb else None
    rounds = torch.empty(B, device=cand.device, dtype=torch.int32)
    lib.sidlsg_edge_hysteresis(ops._p(cand), ops._p(strong), ops._p(edges), ops._p(rgb), ops._p(rounds), B, H, W, ops._s())
    return edges, rgb, rounds


def canny(images_u8_bhwc, low=100, high=200, rgb=False):
    """uint8 [B, H, W, 3] on the device -> EdgeMaps: OpenCV's Canny(img, low, high) per image.  `rgb`: have the hysteresis launch write
    the control image too (else .rgb_u8() makes it on demand)."""
    check_thresholds(low, high)
    images = _images('canny', images_u8_bhwc)
    B, H, W, _ = images.shape
    check_size(H, W)
    cand, strong = classify(images, low, high)
    edges, img, rounds = hysteresis(cand, strong, H, W, want_rgb=rgb)
    return EdgeMaps(edges, H, W, rounds, img)


def pack(images_u8_bhwc, threshold=128):
    """uint8 [B, H, W, 3] -> EdgeMaps: a pixel is set iff any channel is >= threshold (sidlsg_edge_pack_u8)."""
    if int(threshold) != threshold or not 0 <= threshold <= 255:
        raise ValueError(f'pack: threshold = {threshold!r}: expected an integer in 0 .. 255')
    images = _images('pack', images_u8_bhwc)
    B, H, W, _ = images.shape
    bits = torch.empty((B, H, (W + 31) // 32), device=images.device, dtype=torch.int32)
    lib.sidlsg_edge_pack_u8(ops._p(images), ops._p(bits), B, H, W, int(threshold), ops._s())
    return EdgeMaps(bits, H, W)


def match(a, b, tolerance=1):
    """EdgeMaps a, b of one shape -> int64 [B, 4] on the device: |a|, |b|, |a & D_r(b)|, |b & D_r(a)| (sidlsg_edge_match_counts)."""
    check_tolerance(tolerance)
    if (a.B, a.H, a.W) != (b.B, b.H, b.W) or a.bits.device != b.bits.device:
        raise ValueError(f'match: a holds {a.B} maps of {a.H} x {a.W} on {a.bits.device}, b {b.B} of {b.H} x {b.W} on {b.bits.device}: one shape, one device')
    _planes('match', 'a', a.bits, a.B, a.H, a.W), _planes('match', 'b', b.bits, a.B, a.H, a.W)
    counts = torch.empty((a.B, 4), device=a.bits.device, dtype=torch.int64)
    lib.sidlsg_edge_match_counts(ops._p(a.bits), ops._p(b.bits), ops._p(counts), a.B, a.H, a.W, int(tolerance), ops._s())
    return counts


# ---- host rules ----
def _ratio(num, den):
    return num / den if den > 0 else float('nan')


def _f1(p, r):
    if p != p or r != r:
        return float('nan')
    return 0.0 if p + r == 0 else 2 * p * r / (p + r)


def _row(control_edges, output_edges, output_hits, control_hits):
    p, r = _ratio(output_hits, output_edges), _ratio(control_hits, control_edges)
    return dict(control_edges=int(control_edges), output_edges=int(output_edges), output_hits=int(output_hits), control_hits=int(control_hits),
                precision=p, recall=r, f1=_f1(p, r))


def adherence_rows(counts):
    """[B][4] counts of match(control, output) -> one dict per image: control_edges, output_edges, output_hits (output edges within the
    tolerance of a control edge), control_hits, precision = output_hits / output_edges, recall = control_hits / control_edges, f1.  A
    ratio with a zero denominator is NaN; f1 is 0 when both ratios are 0 and NaN when either is NaN."""
    if isinstance(counts, torch.Tensor):
        counts = counts.cpu().tolist()
    # match(control, output) gives |a| = control edges, |b| = output edges, |a & D(b)| = control hits, |b & D(a)| = output hits
    return [_row(int(c[0]), int(c[1]), int(c[3]), int(c[2])) for c in counts]


def aggregate(per_image):
    """Micro-averaged figures of a set from its per-image dicts (a list, or a dict keyed by file name): the four counts are summed over
    the images and precision, recall, f1 computed from the sums, so one image with few edges does not decide the figure (as
    fidelity.aggregate takes PSNR from the mean MSE).  Also f1_macro, the mean f1 over the images where it is defined (NaN when none),
    and images."""
    rows = list(per_image.values()) if isinstance(per_image, dict) else list(per_image)
    if not rows:
        raise ValueError('aggregate: no images')
    out = _row(*(sum(r[k] for r in rows) for k in COUNT_KEYS))
    f1s = [r['f1'] for r in rows if r['f1'] == r['f1']]
    out['f1_macro'] = sum(f1s) / len(f1s) if f1s else float('nan')
    out['images'] = len(rows)
    return out


def format_means(mean):
    return (f'{mean["images"]} images: precision {mean["precision"]:.6g}, recall {mean["recall"]:.6g}, f1 {mean["f1"]:.6g} '
            f'(macro {mean["f1_macro"]:.6g}); {mean["output_edges"]} output and {mean["control_edges"]} control edge pixels')


def score_batch(control, output_u8, low=100, high=200, tolerance=1):
    """control: the EdgeMaps of the control images; output_u8: uint8 [B, H, W, 3] on the device -> one adherence dict per image: the
    output's edge set is canny(output, low, high)."""
    return adherence_rows(match(control, canny(output_u8, low, high), tolerance))
