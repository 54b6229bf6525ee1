"""Canny edge maps and edge matching on the GPU (sid_lsg_amd.edges, csrc/canny.hip) against the numpy / scipy restatement of
tests/canny_ref.py.  Everything is integer: every comparison is equality, on the raw words of the bit planes where padding bits matter.
Each test asserts on the REFERENCE that its case is not trivial before it compares.  tests/test_canny_host.py checks the restatement
itself on cases whose answer can be read off the rule."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import canny_ref as cr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
SENTINEL = 0x5A5A5A5A
GUARD = 64


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def E():
    from sid_lsg_amd import edges
    return edges


def words(mask):
    """bool [.., W] -> the int32 words a kernel must write (padding bits zero)."""
    return E().pack_bits(mask)


def plane(mask, dev):
    return torch.from_numpy(words(mask)).to(dev)


def same_plane(got, want_mask, name):
    got, want = got.cpu().numpy(), words(want_mask)
    assert got.shape == want.shape, f'{name}: shape {got.shape} vs {want.shape}'
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f'{name}: {len(bad)} words differ, first at {bad[0].tolist()}: {got[tuple(bad[0])] & 0xffffffff:#010x} vs {want[tuple(bad[0])] & 0xffffffff:#010x}'


# ---- inputs and references, computed once ----
SHAPES = [(1, 1, 3), (1, 3, 1), (2, 7, 31), (2, 7, 33), (1, 9, 64), (1, 9, 65), (2, 24, 72), (3, 64, 64), (2, 40, 136)]
RECIPES = {(64, 64): (2.0, 2), (40, 136): (2.5, 3)}        # the issue's two images: image 0 of these shapes
_cache = {}


def noise_batch(shape):
    """Distinct images per batch entry; image 0 of the two recipe shapes is the issue's."""
    B, H, W = shape
    imgs = []
    for b in range(B):
        sigma, seed = RECIPES.get((H, W), (1.5, 10 + H + W)) if b == 0 else (1.2 + 0.4 * b, 50 + b + H + W)
        imgs.append(cr.smoothed_noise(H, W, sigma, seed))
    return np.stack(imgs)


def classified(shape, low=100, high=200):
    key = (shape, low, high)
    if key not in _cache:
        imgs = noise_batch(shape)
        refs = [cr.classify_ref(im, low, high) for im in imgs]
        _cache[key] = (imgs, np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs]), np.stack([r[2] for r in refs]))
    return _cache[key]


def border_cases():
    """The hand-made cases of the host test at 40 x 136, the plateau on a tile / word border and on the image border."""
    H, W = 40, 136
    imgs = [cr.step_edge(H, W, x0) for x0 in (64, 32, 1, W - 1)] + [cr.blue_only_edge(H, W, y0) for y0 in (16, 1, H - 1)]
    imgs.append(cr.step_edge(H, W, 64)[:, ::-1].copy())
    return np.stack(imgs)


# ---- classify ----
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_classify_equals_the_reference(dev, shape):
    imgs, cand, strong, _ = classified(shape)
    if shape[1:] in RECIPES:
        e = cr.hysteresis_ref(cand[0], strong[0])
        assert (e & ~strong[0]).sum() >= 50 and (cand[0] & ~e).sum() >= 50 and strong[0].sum() >= 50
    gc, gs = E().classify(torch.from_numpy(imgs).to(dev))
    same_plane(gc, cand, 'cand')
    same_plane(gs, strong, 'strong')


def test_classify_with_thresholds_that_occur(dev):
    shape = (3, 64, 64)
    _, _, _, m = classified(shape)
    vals = np.sort(m[m > 0])
    low, high = int(vals[len(vals) * 4 // 10]), int(vals[len(vals) * 8 // 10])
    assert 0 < low < high and (m == low).sum() >= 1 and (m == high).sum() >= 1
    imgs, cand, strong, _ = classified(shape, low, high)
    assert cand.sum() > 200 and 50 < strong.sum() < cand.sum()
    gc, gs = E().classify(torch.from_numpy(imgs).to(dev), low, high)
    same_plane(gc, cand, 'cand')
    same_plane(gs, strong, 'strong')
    imgs, cand, strong, _ = classified(shape, low, low)         # low == high is admitted
    gc, gs = E().classify(torch.from_numpy(imgs).to(dev), low, low)
    same_plane(gc, cand, 'cand'), same_plane(gs, strong, 'strong')
    assert np.array_equal(cand, strong)


def test_classify_hand_made_cases_on_the_borders(dev):
    imgs = border_cases()
    H, W = imgs.shape[1:3]
    refs = [cr.classify_ref(im) for im in imgs]
    col = lambda x: np.arange(W)[None, :] == x  # noqa: E731
    row = lambda y: np.arange(H)[:, None] == y  # noqa: E731
    for i, x in enumerate((63, 31, 0, W - 2)):       # the left pixel of the plateau (x0 - 1, x0)
        assert np.array_equal(refs[i][0], np.broadcast_to(col(x), (H, W))), i
    for i, y in enumerate((15, 0, H - 2)):           # the upper pixel of the plateau; the edge is in channel B alone
        assert np.array_equal(refs[4 + i][0], np.broadcast_to(row(y), (H, W))), i
    assert np.array_equal(refs[7][0], np.broadcast_to(col(W - 64 - 1), (H, W)))
    gc, gs = E().classify(torch.from_numpy(imgs).to(dev))
    same_plane(gc, np.stack([r[0] for r in refs]), 'cand')
    same_plane(gs, np.stack([r[1] for r in refs]), 'strong')
    # m == low is no candidate, m == high is not strong: every magnitude of image 0 is 800
    for low, high, ncand, nstrong in ((799, 799, H, H), (800, 800, 0, 0), (100, 800, H, 0)):
        gc, gs = E().classify(torch.from_numpy(imgs[:1]).to(dev), low, high)
        c, s, _ = cr.classify_ref(imgs[0], low, high)
        assert c.sum() == ncand and s.sum() == nstrong
        same_plane(gc, c[None], f'cand {low}/{high}'), same_plane(gs, s[None], f'strong {low}/{high}')


# ---- hysteresis, planes fed directly ----
def run_hysteresis(cand, strong, dev, rgb=False):
    B, H, W = cand.shape
    return E().hysteresis(plane(cand, dev), plane(strong, dev), H, W, want_rgb=rgb)


def test_hysteresis_serpentine(dev):
    cand, strong = cr.serpentine(64)
    depth = cr.geodesic_depth(cand, strong)
    assert depth > 2000 and np.array_equal(cr.hysteresis_ref(cand, strong), cand)
    e, _, rounds = run_hysteresis(cand[None], strong[None], dev)
    same_plane(e, cand[None], 'serpentine')
    assert 1 <= int(rounds[0]) <= depth + 1
    print(f'serpentine: {int(rounds[0])} rounds, geodesic depth {depth}')
    gap = (20, 30)
    cand2, _ = cr.serpentine(64, gap=gap)
    want = cr.hysteresis_ref(cand2, strong)
    assert want[:20].sum() == cand2[:20].sum() and 0 < want[20].sum() < 63 and not want[21:].any()
    e, _, _ = run_hysteresis(cand2[None], strong[None], dev)
    same_plane(e, want[None], 'serpentine with a gap')


def percolation(shape, seed):
    """Near the percolation threshold of the 8-connected lattice: large winding components.  The issue's 0.45 / 0.01 keeps more than
    80 % at these seeds; 0.38 / 0.01 was tuned on the reference to keep between 20 % and 80 % of every image."""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    cand = np.stack([rng.random((H, W)) < 0.38 for _ in range(B)])
    strong = np.stack([c & (rng.random((H, W)) < 0.01) for c in cand])
    return cand, strong


@pytest.mark.parametrize('shape,seed', [((3, 24, 33), 10), ((2, 40, 136), 1), ((1, 64, 72), 2), ((1, 768, 768), 3)], ids=lambda v: str(v).replace(' ', ''))
def test_hysteresis_random_planes(dev, shape, seed):
    cand, strong = percolation(shape, seed)
    want = np.stack([cr.hysteresis_ref(c, s) for c, s in zip(cand, strong)])
    for w, c in zip(want, cand):
        assert 0.2 <= w.sum() / c.sum() <= 0.8
    e, rgb, rounds = run_hysteresis(cand, strong, dev, rgb=True)
    same_plane(e, want, 'edges')
    assert np.array_equal(rgb.cpu().numpy(), np.repeat(want[..., None], 3, axis=-1).astype(np.uint8) * 255)
    assert all(1 <= r <= shape[1] * shape[2] + 1 for r in rounds.tolist())
    # idempotence: the edges are their own candidates and seeds; one productive round is not needed
    e2, _, rounds2 = E().hysteresis(e, e, shape[1], shape[2])
    assert torch.equal(e2, e) and rounds2.tolist() == [1] * shape[0]


def test_hysteresis_ignores_strong_outside_cand_and_padding(dev):
    cand, strong = percolation((2, 24, 33), 7)
    want = np.stack([cr.hysteresis_ref(c, s) for c, s in zip(cand, strong)])
    assert (0 < want.sum(axis=(1, 2))).all() and (want.sum(axis=(1, 2)) < cand.sum(axis=(1, 2))).all()
    stray = strong | ~cand                              # every non-candidate pixel claims to be strong
    c, s = plane(cand, dev), plane(stray, dev)
    c[:, :, -1] |= ~0 << 1                              # and the padding bits of both planes are all ones (W = 33: bit 0 is the pixel)
    s[:, :, -1] |= ~0 << 1
    e, rgb, _ = E().hysteresis(c, s, 24, 33, want_rgb=True)
    same_plane(e, want, 'edges')
    assert np.array_equal(rgb.cpu().numpy()[..., 0] == 255, want)
    only_rgb = E().hysteresis(c, s, 24, 33, want_edges=False, want_rgb=True)
    assert only_rgb[0] is None and torch.equal(only_rgb[1], rgb)


# ---- canny end to end ----
@pytest.mark.parametrize('shape', [(2, 7, 33), (3, 64, 64), (2, 40, 136)], ids=lambda s: 'x'.join(map(str, s)))
def test_canny_end_to_end(dev, shape):
    imgs, cand, strong, _ = classified(shape)
    want = np.stack([cr.hysteresis_ref(c, s) for c, s in zip(cand, strong)])
    if shape[1:] in RECIPES:
        assert (want[0] & ~strong[0]).sum() >= 50 and (cand[0] & ~want[0]).sum() >= 50
    x = torch.from_numpy(imgs).to(dev)
    maps = E().canny(x)
    gc, gs = E().classify(x)
    assert torch.equal(maps.bits, E().hysteresis(gc, gs, shape[1], shape[2])[0])
    same_plane(maps.bits, want, 'canny')              # raw words: padding bits are zero
    assert (maps.H, maps.W, maps.B) == (shape[1], shape[2], shape[0]) and maps.rounds.shape == (shape[0],)
    assert np.array_equal(maps.to_bool(), want)
    rgb = maps.rgb_u8().cpu().numpy()
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, np.repeat(want[..., None], 3, axis=-1).astype(np.uint8) * 255)
    assert torch.equal(E().canny(x, rgb=True).rgb_u8(), maps.rgb_u8())
    assert torch.equal(E().pack(maps.rgb_u8()).bits, maps.bits)          # a control image packs back to its edge set


def test_pack(dev):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (3, 9, 65, 3), dtype=np.uint8)
    img[0, 0, :8] = [[127, 127, 127], [128, 0, 0], [0, 128, 0], [0, 0, 128], [255, 255, 255], [0, 0, 0], [127, 128, 127], [127, 127, 0]]
    for t in (128, 1, 255, 0):
        same_plane(E().pack(torch.from_numpy(img).to(dev), t).bits, (img >= t).any(-1), f'pack {t}')


# ---- counts ----
def ref_counts(a, b, r):
    return [cr.match_ref(x, y, r) for x, y in zip(a, b)]


@pytest.mark.parametrize('r', [0, 1, 2, 5])
def test_match_counts_on_the_shifted_pairs(dev, r):
    for shape in ((3, 64, 64), (2, 40, 136)):
        imgs, cand, strong, _ = classified(shape)
        a = np.stack([cr.hysteresis_ref(c, s) for c, s in zip(cand, strong)])
        b = np.roll(a, 1, axis=2)                      # the same maps one column to the right
        r0, r1 = cr.match_ref(a[0], b[0], 0), cr.match_ref(a[0], b[0], 1)
        assert r1[2] - r0[2] >= 100 and r1[3] - r0[3] >= 100          # the tolerance is visible in the counts
        H, W = shape[1:]
        got = E().match(E().EdgeMaps(plane(a, dev), H, W), E().EdgeMaps(plane(b, dev), H, W), r)
        assert got.dtype == torch.int64 and got.cpu().tolist() == ref_counts(a, b, r)


@pytest.mark.parametrize('r', [0, 1, 2, 5])
@pytest.mark.parametrize('W', [33, 72, 136])
def test_match_counts_random_and_borders(dev, W, r):
    B, H = 3, 21
    rng = np.random.default_rng(W)
    a, b = rng.random((B, H, W)) < 0.03, rng.random((B, H, W)) < 0.03
    a[0, 0, :] = True                                  # edges on the image border, every side
    b[0, -1, :] = True
    a[1, :, 0] = b[1, :, -1] = True
    a[2, 0, 0] = a[2, -1, -1] = b[2, 0, -1] = b[2, -1, 0] = True
    a[2, H // 2, W - 1] = True                         # the last pixel of a row and the first of the next are not neighbours
    b[2, H // 2 + 1, 0] = True
    want = ref_counts(a, b, r)
    assert all(w[0] >= 15 and w[1] >= 15 for w in want) and want[0] != want[1] and want[1] != want[2]
    pa, pb = plane(a, dev), plane(b, dev)
    assert E().match(E().EdgeMaps(pa, H, W), E().EdgeMaps(pb, H, W), r).cpu().tolist() == want
    if W % 32:                                         # all-ones padding bits in a hand-built b (and a) must not count or leak
        pa2, pb2 = pa.clone(), pb.clone()
        pb2[:, :, -1] |= ~0 << (W % 32)
        pa2[:, :, -1] |= ~0 << (W % 32)
        assert E().match(E().EdgeMaps(pa, H, W), E().EdgeMaps(pb2, H, W), r).cpu().tolist() == want
        assert E().match(E().EdgeMaps(pa2, H, W), E().EdgeMaps(pb2, H, W), r).cpu().tolist() == want


def test_match_counts_do_not_leak_across_images(dev):
    H, W = 4, 40
    a, b = np.zeros((3, H, W), dtype=bool), np.zeros((3, H, W), dtype=bool)
    a[0, H - 1, :] = True                              # the last row of image 0 against the first row of image 1
    b[1, 0, :] = True
    a[2, 0, 5] = b[2, 1, 6] = True
    for r in (0, 1, 16):
        want = ref_counts(a, b, r)
        assert want[0] == [W, 0, 0, 0] and want[1] == [0, W, 0, 0] and want[2] == [1, 1, int(r > 0), int(r > 0)]
        assert E().match(E().EdgeMaps(plane(a, dev), H, W), E().EdgeMaps(plane(b, dev), H, W), r).cpu().tolist() == want


# ---- refusals ----
class Guarded:
    """`n` elements of `dtype` inside a sentinel-filled buffer, GUARD elements on each side; a refused call leaves ALL of it untouched."""

    def __init__(self, n, dtype, dev):
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL if dtype != torch.uint8 else 0x5A, device=dev, dtype=dtype)
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()
        self.fill = self.buf[0].item()

    def untouched(self):
        return bool((self.buf == self.fill).all())


def test_refusals_leave_the_outputs_untouched(dev):
    from sid_lsg_amd._lib import lib
    B, H, W = 2, 8, 40
    Wd = 2
    img = torch.zeros((B, H, W, 3), device=dev, dtype=torch.uint8)
    pl = torch.zeros((B, H, Wd), device=dev, dtype=torch.int32)
    outs = [Guarded(B * H * Wd, torch.int32, dev) for _ in range(2)]
    rgb, rounds, counts = Guarded(B * H * W * 3, torch.uint8, dev), Guarded(B, torch.int32, dev), Guarded(B * 4, torch.int64, dev)
    i, p, s = img.data_ptr(), pl.data_ptr(), 0
    o0, o1 = outs[0].ptr, outs[1].ptr
    classify, hyst, pack, match = (getattr(lib, n).raw for n in ('sidlsg_canny_classify_u8', 'sidlsg_edge_hysteresis', 'sidlsg_edge_pack_u8',
                                                                 'sidlsg_edge_match_counts'))
    calls = {
        'classify NULL images': lambda: classify(None, o0, o1, B, H, W, 100, 200, s),
        'classify NULL cand': lambda: classify(i, None, o1, B, H, W, 100, 200, s),
        'classify NULL strong': lambda: classify(i, o0, None, B, H, W, 100, 200, s),
        'classify B 0': lambda: classify(i, o0, o1, 0, H, W, 100, 200, s),
        'classify H -1': lambda: classify(i, o0, o1, B, -1, W, 100, 200, s),
        'classify W 0': lambda: classify(i, o0, o1, B, H, 0, 100, 200, s),
        'classify low > high': lambda: classify(i, o0, o1, B, H, W, 201, 200, s),
        'classify low < 0': lambda: classify(i, o0, o1, B, H, W, -1, 200, s),
        'classify high < 0': lambda: classify(i, o0, o1, B, H, W, -2, -1, s),
        'hysteresis NULL cand': lambda: hyst(None, p, o0, rgb.ptr, rounds.ptr, B, H, W, s),
        'hysteresis NULL strong': lambda: hyst(p, None, o0, rgb.ptr, rounds.ptr, B, H, W, s),
        'hysteresis both outputs NULL': lambda: hyst(p, p, None, None, rounds.ptr, B, H, W, s),
        'hysteresis B 0': lambda: hyst(p, p, o0, rgb.ptr, rounds.ptr, 0, H, W, s),
        'hysteresis H 0': lambda: hyst(p, p, o0, rgb.ptr, rounds.ptr, B, 0, W, s),
        'hysteresis W -3': lambda: hyst(p, p, o0, rgb.ptr, rounds.ptr, B, H, -3, s),
        'hysteresis 1024 x 1024': lambda: hyst(p, p, o0, rgb.ptr, rounds.ptr, 1, 1024, 1024, s),
        'hysteresis 769 x 768': lambda: hyst(p, p, o0, rgb.ptr, rounds.ptr, 1, 769, 768, s),
        'pack NULL images': lambda: pack(None, o0, B, H, W, 128, s),
        'pack NULL bits': lambda: pack(i, None, B, H, W, 128, s),
        'pack B -1': lambda: pack(i, o0, -1, H, W, 128, s),
        'pack H 0': lambda: pack(i, o0, B, 0, W, 128, s),
        'pack W 0': lambda: pack(i, o0, B, H, 0, 128, s),
        'pack threshold 256': lambda: pack(i, o0, B, H, W, 256, s),
        'pack threshold -1': lambda: pack(i, o0, B, H, W, -1, s),
        'match NULL a': lambda: match(None, p, counts.ptr, B, H, W, 1, s),
        'match NULL b': lambda: match(p, None, counts.ptr, B, H, W, 1, s),
        'match NULL counts': lambda: match(p, p, None, B, H, W, 1, s),
        'match B 0': lambda: match(p, p, counts.ptr, 0, H, W, 1, s),
        'match H 0': lambda: match(p, p, counts.ptr, B, 0, W, 1, s),
        'match W -1': lambda: match(p, p, counts.ptr, B, H, -1, 1, s),
        'match r -1': lambda: match(p, p, counts.ptr, B, H, W, -1, s),
        'match r 17': lambda: match(p, p, counts.ptr, B, H, W, 17, s),
    }
    for name, call in calls.items():
        assert call() == EINVAL, name
    torch.cuda.synchronize()
    for name, g in (('cand / edges / bits', outs[0]), ('strong', outs[1]), ('rgb', rgb), ('rounds', rounds), ('counts', counts)):
        assert g.untouched(), f'{name}: a refused call wrote'
    assert lib.sidlsg_edge_hysteresis_lds_bytes.raw(768, 768) == 147456 and lib.sidlsg_edge_hysteresis_lds_bytes.raw(1024, 1024) == EINVAL
    # admitted calls into the same guarded buffers write their extent and nothing else
    assert classify(i, o0, o1, B, H, W, 100, 200, s) == 0 and hyst(p, p, o0, rgb.ptr, rounds.ptr, B, H, W, s) == 0
    assert match(p, p, counts.ptr, B, H, W, 16, s) == 0
    torch.cuda.synchronize()
    for g, n in ((outs[0], B * H * Wd), (outs[1], B * H * Wd), (rgb, B * H * W * 3), (rounds, B), (counts, B * 4)):
        assert (g.buf[:GUARD] == g.fill).all() and (g.buf[GUARD + n:] == g.fill).all()
    assert (outs[0].buf[GUARD:GUARD + B * H * Wd] == 0).all() and (rgb.buf[GUARD:GUARD + B * H * W * 3] == 0).all()
    assert rounds.buf[GUARD:GUARD + B].tolist() == [1, 1] and (counts.buf[GUARD:GUARD + 4 * B] == 0).all()


def test_python_refusals_on_the_gpu(dev):
    big = torch.zeros((1, 1024, 1024, 3), device=dev, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r'canny: the two bit planes of a 1024 x 1024 image take 262144 bytes, above the limit of 147456 bytes'):
        E().canny(big)
    pl = torch.zeros((1, 1024, 32), device=dev, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'hysteresis: the two bit planes of a 1024 x 1024 image take 262144 bytes, above the limit of 147456'):
        E().hysteresis(pl, pl, 1024, 1024)
    img = torch.zeros((1, 8, 8, 3), device=dev, dtype=torch.uint8)
    with pytest.raises(ValueError, match='low = 5 is above high = 4'):
        E().canny(img, 5, 4)
    with pytest.raises(ValueError, match='low = -1'):
        E().classify(img, -1, 4)
    a, b = E().pack(img), E().pack(torch.zeros((1, 8, 9, 3), device=dev, dtype=torch.uint8))
    for r in (-1, 17):
        with pytest.raises(ValueError, match=f'match: tolerance = {r}'):
            E().match(a, a, r)
    with pytest.raises(ValueError, match='match: a holds 1 maps of 8 x 8 .* b 1 of 8 x 9'):
        E().match(a, b)
    with pytest.raises(ValueError, match='hysteresis: strong: expected int32'):
        E().hysteresis(a.bits, b.bits.repeat(1, 1, 2), 8, 8)


# ---- command line ----
def _png(path):
    import PIL.Image
    return np.asarray(PIL.Image.open(path).convert('RGB'))


def _rows_ref(ctl, out, r):
    """The adherence figures from two bool maps, written out independently of sid_lsg_amd.edges."""
    na, nb, ha, hb = cr.match_ref(ctl, out, r)
    nan = float('nan')
    p, rc = (hb / nb if nb else nan), (ha / na if na else nan)
    f1 = nan if (p != p or rc != rc) else (0.0 if p + rc == 0 else 2 * p * rc / (p + rc))
    return dict(control_edges=na, output_edges=nb, output_hits=hb, control_hits=ha, precision=p, recall=rc, f1=f1)


def _same(a, b):
    assert a.keys() == b.keys(), (a, b)
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, float) and math.isnan(x):
            assert isinstance(y, float) and math.isnan(y), (k, a, b)
        elif k in ('f1', 'f1_macro'):
            assert x == pytest.approx(y, rel=1e-12), (k, a, b)
        else:
            assert x == y, (k, a, b)


def test_generate_onestep_preprocess_and_adherence(dev, tmp_path):
    """One teacher run on random:tiny with random:controlnet at 64 x 64 from two photographs of other sizes: control_adherence.json
    equals what the reference computes from the PNGs read back and the reference Canny of load_init_image's crop; the same run fed
    the finished maps, without the new options, writes the same PNG bytes and no JSON; tools/edge_adherence.py prints the same mean."""
    import PIL.Image
    from click.testing import CliRunner
    import generate_onestep
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import edge_adherence
    low, high, tol = 10, 20, 1
    prompts = tmp_path / 'prompts.txt'
    prompts.write_text('a red cube\na blue sphere\n')
    photos, maps_dir = tmp_path / 'photos', tmp_path / 'maps'
    photos.mkdir(), maps_dir.mkdir()
    for i, (h, w) in enumerate(((80, 100), (90, 70))):
        PIL.Image.fromarray(cr.smoothed_noise(h, w, 2.0, 20 + i)).save(str(photos / f'photo{i}.png'))
    ctl = []
    for i in range(2):
        crop = generate_onestep.load_init_image(str(photos / f'photo{i}.png'), 64)
        assert crop.shape == (64, 64, 3)
        ctl.append(cr.canny_ref(crop, low, high))
        assert ctl[-1].sum() > 200
        PIL.Image.fromarray(np.repeat(ctl[-1][..., None], 3, axis=-1).astype(np.uint8) * 255).save(str(maps_dir / f'photo{i}.png'))
    common = ['--network', 'teacher', '--repo_id', 'random:tiny', '--teacher_steps', '2', '--seeds', '0-2', '--resolution', '64',
              '--text_prompts', str(prompts), '--controlnet', 'random:controlnet']
    out_a, out_b = tmp_path / 'a', tmp_path / 'b'
    new = ['--control_images', str(photos), '--control_preprocess', 'canny', '--control_adherence', '1', '--canny_low', str(low), '--canny_high', str(high)]
    ra = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out_a)] + common + new, catch_exceptions=False)
    assert ra.exit_code == 0 and 'Control adherence over 3 images' in ra.output, ra.output
    rb = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out_b)] + common + ['--control_images', str(maps_dir)], catch_exceptions=False)
    assert rb.exit_code == 0 and 'adherence' not in rb.output and 'Canny' not in rb.output, rb.output
    names = ['000000.png', '000001.png', '000002.png']
    assert sorted(os.listdir(out_b)) == names and sorted(os.listdir(out_a)) == names + ['control_adherence.json']
    for n in names:
        assert (out_a / n).read_bytes() == (out_b / n).read_bytes(), n
    report = json.load(open(out_a / 'control_adherence.json'))
    want = {n: _rows_ref(ctl[k % 2], cr.canny_ref(_png(str(out_a / n)), low, high), tol) for k, n in enumerate(names)}
    assert sum(w['output_edges'] for w in want.values()) > 0
    assert list(report['per_image']) == names
    for n in names:
        _same(report['per_image'][n], want[n])
    sums = [sum(w[k] for w in want.values()) for k in ('control_edges', 'output_edges', 'control_hits', 'output_hits')]
    p, rc = (sums[3] / sums[1] if sums[1] else float('nan')), sums[2] / sums[0]
    f1s = [w['f1'] for w in want.values() if w['f1'] == w['f1']]
    mean = dict(control_edges=sums[0], output_edges=sums[1], output_hits=sums[3], control_hits=sums[2], precision=p, recall=rc,
                f1=float('nan') if p != p else (0.0 if p + rc == 0 else 2 * p * rc / (p + rc)),
                f1_macro=sum(f1s) / len(f1s) if f1s else float('nan'), images=3)
    _same(report['mean'], mean)
    opts = report['options']
    assert (opts['canny_low'], opts['canny_high'], opts['edge_tolerance'], opts['control_preprocess']) == (low, high, tol, 'canny')
    rt = CliRunner().invoke(edge_adherence.main, ['--control', str(maps_dir), '--images', str(out_b), '--canny_low', str(low), '--canny_high', str(high)],
                            catch_exceptions=False)
    assert rt.exit_code == 0, rt.output
    tool = json.loads(rt.output)
    _same(tool['mean'], mean)
    assert list(tool['per_image']) == names


def test_canny_edges_tool_writes_the_control_images(dev, tmp_path):
    import PIL.Image
    from click.testing import CliRunner
    import generate_onestep
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import canny_edges
    photos, out = tmp_path / 'photos', tmp_path / 'ctl'
    photos.mkdir()
    for i, (h, w) in enumerate(((50, 64), (40, 40), (33, 70))):
        PIL.Image.fromarray(cr.smoothed_noise(h, w, 1.5, 30 + i)).save(str(photos / f'p{i}.png'))
    res = CliRunner().invoke(canny_edges.main, ['--images', str(photos), '--out', str(out), '--resolution', '40', '--batch', '2'], catch_exceptions=False)
    assert res.exit_code == 0 and '3 control image(s) of 40 x 40' in res.output, res.output
    assert sorted(os.listdir(out)) == ['p0.png', 'p1.png', 'p2.png']
    for i in range(3):
        want = cr.canny_ref(generate_onestep.load_init_image(str(photos / f'p{i}.png'), 40))
        assert want.sum() > 50
        assert np.array_equal(_png(str(out / f'p{i}.png')), np.repeat(want[..., None], 3, axis=-1).astype(np.uint8) * 255)
