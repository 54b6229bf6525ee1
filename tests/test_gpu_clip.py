"""CLIP score on the GPU: the three kernels of csrc/clip.hip against fp64 restatements, the ViT image tower against
transformers.CLIPModel (tests/golden/clip_ref.npz, tools/make_clip_goldens.py), the detector contract and the metric end to end.

Measured on the MI355X (the figures the 4x assertions below are built on; DESIGN.md carries the same numbers):
  gelu, fp32 kernel, worst error in ulps of the result on the grid of test_gelu: quick_gelu 17.02 (x = -9.91), exact GELU 75.74
    (x = -9.40) -- both in the negative tail, where the result is exp(-17) / erfc(6.6) small and the ONE rounding of the argument
    (1.702 x, x / sqrt 2) is amplified by its size; within |x| <= 3 both stay below 4 ulps
  tower, fp32 mode, worst relative l2 per image against the golden image_embeds: (a) 2.14e-6, (b) 3.45e-6
  tower, bf16 mode, worst |cosine - golden cosine| of the three pairs: (a) 4.20e-3, (b) 3.40e-3
clip_patches: fp32 kernel at most 4.4e-6 from the fp64 restatement (bound 1e-5); the bf16 kernel fills 0.998 of its bound, which is
its one rounding (half a bf16 ulp).
"""
import json
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clip_ref_util import MEAN, RESIZE_CASES, STD, case_images, golden, patch_rows64, pixel_values64, write_clip_dir

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32

# measured on the MI355X (module docstring); every assertion that uses one allows 4x the figure
GELU_ULPS = {'quick_gelu': 17.02, 'gelu': 75.74}
TOWER_F32_REL_L2 = {'a': 2.14e-6, 'b': 3.45e-6}
TOWER_BF16_COS = {'a': 4.20e-3, 'b': 3.40e-3}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ref(golden_dir):
    return golden(golden_dir)


@pytest.fixture(scope='module')
def dirs(ref, tmp_path_factory):
    root = tmp_path_factory.mktemp('clip')
    return {tag: write_clip_dir(ref, tag, root / tag) for tag in 'ab'}


def _ulp(r, mant, emin):
    """Spacing of the floating-point numbers with `mant` mantissa bits and smallest exponent `emin` around r (fp64 tensor)."""
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -300)))
    return torch.exp2((e - mant).clamp_min(emin))


# ---- clip_patches ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def patch_refs():
    """name -> (images, [B, G*G, 3*P*P] fp64 rows of the restated pixel_values), computed once."""
    out = {}
    for name, B, H, W, R, P in RESIZE_CASES:
        img = case_images(name, B, H, W)
        out[name] = (img, patch_rows64(pixel_values64(img, R), P))
    return out


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name,B,H,W,R,P', RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_clip_patches(dev, patch_refs, name, B, H, W, R, P, dtype):
    """A 16-term fp32 sum of values in [0, 1] with sum |w| <= 1.25^2, divided by std >= 0.26: 1e-5 absolute against the fp64
    restatement for the fp32 kernel; the bf16 kernel adds half a bf16 ulp of the result."""
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    img, want = patch_refs[name]
    G, K, kp = R // P, 3 * P * P, ops.clip_patch_width(P)
    T = 1 + G * G
    assert kp % 8 == 0 and 0 <= kp - K < 8
    d_img = img.to(dev)
    out = torch.full((B * T, kp), float('nan'), device=dev, dtype=dtype)
    ops._fn('clip_patches_u8', dtype)(d_img.data_ptr(), out.data_ptr(), B, H, W, R, P, kp, *MEAN, *STD, ops._s())
    torch.cuda.synchronize()
    got = out.view(B, T, kp).cpu()
    assert not torch.isnan(got).any(), 'every element of the output is written'
    assert (got[:, 0] == 0).all(), 'the class-token row of every image is zero'
    assert (got[:, :, K:] == 0).all(), 'the pad columns are zero'
    body = got[:, 1:, :K].double()
    err = (body - want).abs()
    # half a bf16 ulp is 2^-8 of the power of two below |v|, i.e. between 2^-9 |v| (top of a binade) and 2^-8 |v| (bottom): a plain
    # `2^-9 |v|` is missed by the correctly rounded value itself over the lower half of every binade, so the ulp is formed exactly
    bound = 1e-5 + (0.5 * _ulp(want, 7, -133) if dtype == BF16 else 0.0)
    print(f'{name} {dtype}: max |kernel - fp64 restatement| = {float(err.max()):.3e}, worst share of the bound {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all())
    assert torch.equal(ops.clip_patches(d_img, R, P, dtype).cpu(), got.view(B * T, kp)), 'the public wrapper is the same launch'
    if name == 'identity_32' and dtype == F32:
        # taps (0, 1, 0, 0) exactly: the fp32 lines of the wrapper, bit for bit
        x = (img.to(F32) / 255. - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
        assert torch.equal(got[:, 1:, :K], F.unfold(x, P, stride=P).transpose(1, 2))


def test_clip_patches_refusals(dev):
    from sid_lsg_amd import ops
    img = torch.zeros(1, 3, 16, 16, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match='multiple of the patch size'):
        ops.clip_patches(img, 30, 8)
    with pytest.raises(RuntimeError, match=r'uint8 \[B, 3, H, W\]'):
        ops.clip_patches(img[:, :2], 32, 8)
    with pytest.raises(RuntimeError, match='uint8'):
        ops.clip_patches(img.float(), 32, 8)
    out = torch.empty(5 * 592, device=dev)
    with pytest.raises(RuntimeError, match='sidlsg_clip_patches_u8_f32 failed'):        # Kp not a multiple of 8: no launch
        ops._fn('clip_patches_u8', F32)(img.data_ptr(), out.data_ptr(), 1, 16, 16, 28, 14, 588, *MEAN, *STD, ops._s())


# ---- gelu ----------------------------------------------------------------------------------------------------------------------
def _gelu_grid():
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.linspace(-10, 10, 4005), torch.randn(2000, generator=g) * 3,
                   torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1e-38, -1e-38, float('inf'), float('-inf'), float('nan'),
                                 10.0, -10.0, 1e-20, -1e-20])])
    assert x.numel() % 8 == 4         # the scalar tail behind the last group of 8 runs too
    return x


def _gelu64(x, mode):
    x = x.double()
    if mode == 'quick_gelu':
        return x * torch.sigmoid(1.702 * x)
    return 0.5 * x * torch.special.erfc(-x * 0.5 ** 0.5)        # = x Phi(x); erfc keeps the negative tail in fp64 too


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('mode', ['quick_gelu', 'gelu'])
def test_gelu(dev, mode, dtype):
    """fp32 kernel: within 4x the measured worst error (GELU_ULPS, ulps of the result: the device's expf / erfcf error is not
    something the project records elsewhere); the bf16 kernel evaluates the same fp32 and adds half a bf16 ulp at its one rounding."""
    from sid_lsg_amd import ops
    x = _gelu_grid().to(dtype)
    want = _gelu64(x, mode)
    got = ops.gelu(x.to(dev), mode)
    assert got.dtype == dtype and got.shape == x.shape
    got = got.cpu().double()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), 'NaN in (x = NaN, and -inf * 0 at x = -inf) is NaN out, and nothing else is'
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf])
    fin = ~(nan | inf)
    err = (got - want).abs()[fin]
    u32 = _ulp(want[fin], 23, -149)
    if dtype == F32:
        worst = float((err / u32).max())
        print(f'gelu {mode} fp32: worst error {worst:.2f} ulps of the result (at x = {float(x[fin][(err / u32).argmax()]):.6g})')
        bound = 4 * GELU_ULPS[mode] * u32
    else:
        bound = 4 * GELU_ULPS[mode] * u32 + 0.5 * _ulp(want[fin], 7, -133)
        print(f'gelu {mode} bf16: worst share of the bound {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all())
    assert float(got[x == 0].abs().max()) == 0.0


# ---- clip_score ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('B,Fd', [(1, 24), (5, 24), (5, 32), (1, 1024), (5, 1024), (5, 30)])
def test_clip_score(dev, B, Fd, dtype):
    """F.normalize and the row dot product in fp64.  Cosine: an F-term fp32 dot product, F * 2^-24 relative to sum |a_i b_i|.
    Features: x / max(|x|, 1e-12) with |x|^2 an F-term fp32 sum (F / 2 roundings on the norm), a square root and a division."""
    from sid_lsg_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + Fd)
    img, txt = (torch.randn(B, Fd, generator=g).to(dtype) for _ in range(2))
    if B > 1:
        img[1] = 0                     # the eps path of F.normalize
        txt[3] *= 1e-3
    feats, cos = ops.clip_score(img.to(dev), txt.to(dev))
    assert feats.dtype == F32 and feats.shape == (B, 2 * Fd) and cos.dtype == F32 and cos.shape == (B,)
    a, b = (F.normalize(t.double(), dim=-1, eps=1e-12) for t in (img, txt))
    want = torch.cat([a, b], 1)
    u = 2.0 ** -24
    ferr = (feats.cpu().double() - want).abs()
    assert bool((ferr <= (Fd / 2 + 2) * u * want.abs()).all()), float((ferr / want.abs().clamp_min(1e-30)).max() / u)
    cerr = (cos.cpu().double() - (a * b).sum(-1)).abs()
    cbound = Fd * u * (a * b).abs().sum(-1)
    print(f'clip_score B={B} F={Fd} {dtype}: cosine error / bound = {float((cerr / cbound.clamp_min(1e-300)).max()):.3f}')
    assert bool((cerr <= cbound).all())
    if B > 1:
        assert float(feats[1, :Fd].abs().max()) == 0 and float(cos[1]) == 0


# ---- the tower against transformers ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def towers(dev, dirs):
    from sid_lsg_amd.clip import load_clip
    return {(tag, dt): load_clip(dirs[tag], dev, compute_dtype=dt) for tag in 'ab' for dt in (F32, BF16)}


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_tower_fp32_matches_transformers(dev, ref, towers, tag):
    """fp32 mode against the golden image_embeds (transformers on the CPU): relative l2 per image.  Reduction order differs, nothing
    else should: 4x the measured value, the margin of the teacher-sampler tests."""
    det = towers[(tag, F32)]
    with torch.no_grad():
        emb = det.vision(torch.from_numpy(ref[f'{tag}/images']).to(dev))
    assert emb.dtype == F32 and emb.shape == ref[f'{tag}/image_embeds'].shape
    got = F.normalize(emb.cpu().double(), dim=-1)
    want = torch.from_numpy(ref[f'{tag}/image_embeds']).double()
    rel = (got - want).norm(dim=-1) / want.norm(dim=-1)
    print(f'tower ({tag}) fp32: relative l2 per image {rel.tolist()}')
    assert float(rel.max()) <= 4 * TOWER_F32_REL_L2[tag]


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_tower_bf16_cosines(dev, ref, towers, tag):
    from sid_lsg_amd import ops
    det = towers[(tag, BF16)]
    with torch.no_grad():
        emb = det.vision(torch.from_numpy(ref[f'{tag}/images']).to(dev))
        txt = det.text_embeds_from_ids(torch.from_numpy(ref[f'{tag}/ids_padeos']))
        feats, cos = ops.clip_score(emb, txt.contiguous())
    err = (cos.cpu().double() - torch.from_numpy(ref[f'{tag}/cosines']).double()).abs()
    print(f'tower ({tag}) bf16: |cosine - golden| {err.tolist()}')
    assert float(err.max()) <= 4 * TOWER_BF16_COS[tag]
    # the text half is fp32 torch: the bound of the host test
    torch.testing.assert_close(feats[:, feats.shape[1] // 2:].cpu(), torch.from_numpy(ref[f'{tag}/text_embeds']), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_tokens_do_not_depend_on_the_batch(dev, ref, towers, tag, dt):
    """The class-token / position-embedding `res` operand is laid out per image: image i of a batch of 3 gets the tokens it gets alone."""
    vis = towers[(tag, dt)].vision
    images = torch.from_numpy(ref[f'{tag}/images']).to(dev)
    with torch.no_grad():
        three = vis.embed(images).view(3, vis.tokens, -1).clone()
        for i in range(3):
            one = vis.embed(images[i:i + 1]).view(vis.tokens, -1)
            assert torch.equal(one, three[i]), i
        # row 0 of every image: no patch, so exactly class embedding + position 0 (rounded to the compute dtype)
        m = vis.masters
        cls = (m['vision_model.embeddings.position_embedding.weight'][0] + m['vision_model.embeddings.class_embedding']).to(dt)
        assert all(torch.equal(three[i, 0], cls) for i in range(3))
    with pytest.raises(RuntimeError, match='no_grad'):
        vis(images)


# ---- detector and metric ---------------------------------------------------------------------------------------------------------
def test_detector_contract(dev, ref, towers):
    from sid_lsg_amd.metrics import clip_score_from_features
    det = towers[('a', BF16)]
    images = torch.from_numpy(ref['a/images']).to(dev)
    texts = ['a cat', 'two dogs on a hill', 'x']
    f = det(images, texts=texts, div255=True)
    Fd = det.vision.cfg.projection_dim
    assert f.dtype == F32 and f.shape == (3, 2 * Fd)
    for half in (f[:, :Fd], f[:, Fd:]):
        torch.testing.assert_close(half.norm(dim=-1).cpu(), torch.ones(3), rtol=0, atol=1e-6)
    s = det.scores(images, texts)
    assert s.shape == (3,) and s.dtype == F32
    assert abs(clip_score_from_features(f) - float(s.mean())) <= 1e-6
    with pytest.raises(ValueError, match='div255'):
        det(images, texts=texts, div255=False)
    with pytest.raises(ValueError, match='one text per image'):
        det(images, texts=texts[:2])


def test_fid_clip_test_end_to_end(dev, dirs):
    """calc_metric('fid_clip_test') with CLIP directories under both names: 6 samples in batches of 4 + 2; both scores equal the
    values recomputed from the same images and captions through the detectors.  Without the paths both stay NaN, as before."""
    from sid_lsg_amd import metrics
    from sid_lsg_amd.clip import load_clip
    from sid_lsg_amd.sd_util import load_sd15, sid_sd_sampler
    unet, vae, sched, te, tok = load_sd15('random:tiny', None, dev, BF16)
    unet.eval().requires_grad_(False)
    G = partial(sid_sd_sampler, unet=unet, noise_scheduler=sched, text_encoder=te, tokenizer=tok, resolution=64, dtype=F32,
                return_images=True, vae=vae, train_sampler=False)
    seen = dict(texts=[], images=[])

    def G_rec(latents, contexts, init_timesteps):
        seen['texts'].append(list(contexts))
        return G(latents=latents, contexts=contexts, init_timesteps=init_timesteps)
    proj = torch.randn(3 * 8 * 8, 12, generator=torch.Generator().manual_seed(1)).to(dev)

    def inception(img, return_features=True):
        seen['images'].append(img.clone())
        return F.adaptive_avg_pool2d(img.float(), 8).flatten(1) @ proj
    prompts = ['a red cube', 'blue sphere', 'two cats', 'a dog on a hill', 'green', 'the sea at night', 'a b c']
    kw = dict(G=G_rec, prompts=prompts, resolution=64, init_timestep=625, detector=inception, real_stats=(np.zeros(12), np.eye(12)),
              device=dev, num_test=6, batch_gen=4, detector_size=96)
    res = metrics.calc_metric('fid_clip_test', open_clip_detector=dirs['a'], metric_clip_path=dirs['b'], **kw).results
    assert [len(t) for t in seen['texts']] == [4, 2] and [tuple(i.shape) for i in seen['images']] == [(4, 3, 96, 96), (2, 3, 96, 96)]
    assert np.isfinite(res.open_clipscore_30k) and np.isfinite(res.clipscore30k) and np.isfinite(res.fid30k_full)
    det_a, det_b = load_clip(dirs['a'], dev), load_clip(dirs['b'], dev)
    oc, cs = [], []
    for img, texts in zip(seen['images'], seen['texts']):
        oc += [metrics.clip_score_from_features(det_a(img, texts=texts, div255=True))] * len(texts)
        cs.append(det_b.scores(img, texts).cpu().double())
    print(f'open_clipscore_30k {res.open_clipscore_30k:.6f}  clipscore30k {res.clipscore30k:.6f}')
    assert abs(res.open_clipscore_30k - float(np.mean(oc))) <= 1e-7
    assert abs(res.clipscore30k - float(torch.cat(cs).mean())) <= 1e-7
    assert abs(res.open_clipscore_30k - res.clipscore30k) > 1e-4, 'two different models were scored'
    seen['texts'].clear(), seen['images'].clear()
    none = metrics.calc_metric('fid_clip_test', **kw).results
    assert np.isnan(none.open_clipscore_30k) and np.isnan(none.clipscore30k) and none.fid30k_full == res.fid30k_full
    cfg = json.load(open(dirs['a'] + '/config.json'))
    assert cfg['vision_config']['image_size'] == 32
