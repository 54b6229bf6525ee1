"""HPSv2 on the GPU: sidlsg_pil_patches_u8 against Pillow + the torch ToTensor / Normalize lines bit for bit
(tests/golden/hps_ref.npz, tools/make_hps_goldens.py), the tower loaded from an open_clip-layout checkpoint against
transformers.CLIPModel, and the two command lines end to end.

Measured on the MI355X against the transformers golden (the figures the 4x assertions below are built on; DESIGN.md carries the same):
  tower from load_open_clip, preprocess='pil', fp32 mode, worst relative l2 per image against the golden image_embeds: 1.26e-6
    (the three images: 1.12e-6, 1.25e-6, 1.04e-6)
  the same tower in bf16 mode, worst |cosine - golden cosine| of the three pairs: 1.72e-3
    (1.72e-3, 3.41e-4, 1.22e-3)
  HIP text tower (fp32) against the golden text_embeds, relative l2 per row: 1.20e-6, 1.15e-6, 1.99e-6; against the torch tower: 1.44e-6,
    1.64e-6, 4.95e-7 -- inside the 4 x 1.18e-6 tests/test_gpu_text_hip.py allows
  pil_patches: 0 differing elements on every shape, fp32 and bf16
"""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hps_ref_util import CASES, MEAN, STD, STYLES, golden, pixel_values, write_checkpoint, write_prompts, write_tokenizer

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
EINVAL = -22

# measured on the MI355X (module docstring); every assertion that uses one allows 4x the figure
TOWER_F32_REL_L2 = 1.26e-6
TOWER_BF16_COS = 1.72e-3
F32_CEILING = 4 * 3.45e-6           # the largest bound tests/test_gpu_clip.py holds for a tower of this size: beyond it is a bug
TEXT_F32_REL_L2 = 1.18e-6           # tests/test_gpu_text_hip.py: HIP text tower against the golden text_embeds, asserted at 4x


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ref(golden_dir):
    return golden(golden_dir)


@pytest.fixture(scope='module')
def files(ref, tmp_path_factory):
    root = tmp_path_factory.mktemp('hps')
    return dict(checkpoint=write_checkpoint(ref, root / 'hps_tiny.pt', wrap=True), tokenizer=write_tokenizer(root / 'tokenizer'), root=root)


# ---- the patch kernel ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def patch_refs(ref):
    """name -> (uint8 source images, [B, G*G, 3*P*P] fp32 unfold of the golden pixel_values), computed once."""
    return {name: (torch.from_numpy(ref[f'src/{name}']), F.unfold(pixel_values(ref, name), P, stride=P).transpose(1, 2).contiguous())
            for name, B, H, W, R, P in CASES}


def _raw_args(ops, img, out, B, H, W, R, P, kp):
    t, hk, vk, band_rows = ops._pil_plan(H, W, R, P, img.device)
    return [img.data_ptr(), out.data_ptr(), B, H, W, R, P, kp, t['hbounds'].data_ptr(), t['hcoef'].data_ptr(), hk, t['vbounds'].data_ptr(),
            t['vcoef'].data_ptr(), vk, band_rows, *MEAN, *STD, ops._s()]


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name,B,H,W,R,P', CASES, ids=[c[0] for c in CASES])
def test_pil_patches_is_bit_equal_to_pillow_and_torch(dev, patch_refs, name, B, H, W, R, P, dtype):
    """No tolerance: the integer stage is exact and the float tail is two IEEE divisions and a subtraction; bf16 is that rounded once."""
    from sid_lsg_amd import ops
    img, want = patch_refs[name]
    G, K, kp = R // P, 3 * P * P, ops.clip_patch_width(P)
    T = 1 + G * G
    d_img = img.to(dev)
    out = torch.full((B * T, kp), float('nan'), device=dev, dtype=dtype)
    ops._fn('pil_patches_u8', dtype)(*_raw_args(ops, d_img, out, B, H, W, R, P, kp))
    torch.cuda.synchronize()
    got = out.view(B, T, kp).cpu()
    assert not torch.isnan(got).any(), 'every element of the output is written'
    assert (got[:, 0] == 0).all(), 'the class-token row of every image is zero'
    assert (got[:, :, K:] == 0).all(), 'the pad columns are zero'
    body = got[:, 1:, :K]
    expect = want if dtype == F32 else want.to(BF16)
    bad = int((body != expect).sum())
    print(f'{name} {dtype}: {bad} of {body.numel()} elements differ from Pillow + ToTensor + Normalize')
    assert torch.equal(body, expect)
    assert torch.equal(ops.pil_patches(d_img, R, P, dtype).cpu(), got.view(B * T, kp)), 'the public wrapper is the same launch'
    for b in range(B):
        one = ops.pil_patches(d_img[b:b + 1], R, P, dtype).cpu()
        assert torch.equal(one, got[b]), f'image {b} alone equals image {b} of the batch'


def test_pil_patches_refusals(dev):
    """SIDLSG_EINVAL from the entry point itself, in front of any launch (the raw return code, no exception wrapper)."""
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    B, H, W, R, P = 1, 40, 40, 32, 8
    kp = ops.clip_patch_width(P)
    img = torch.zeros(B, 3, H, W, dtype=torch.uint8, device=dev)
    out = torch.zeros(B * 17 * kp + 8, device=dev, dtype=F32)
    base = _raw_args(ops, img, out, B, H, W, R, P, kp)
    names = ['images', 'out', 'B', 'H', 'W', 'R', 'P', 'Kp', 'hbounds', 'hcoef', 'hk', 'vbounds', 'vcoef', 'vk', 'band_rows', 'mean0', 'mean1',
             'mean2', 'std0', 'std1', 'std2', 'stream']

    def call(fn=lib.sidlsg_pil_patches_u8_f32, **edit):
        args = list(base)
        for k, v in edit.items():
            args[names.index(k)] = v
        return fn.raw(*args)
    assert call() == 0 and call(lib.sidlsg_pil_patches_u8) == 0
    torch.cuda.synchronize()
    cases = dict(R=dict(R=30), kp_mod=dict(Kp=kp + 4), kp_small=dict(Kp=3 * P * P - 8), std0=dict(std0=0.0), std2=dict(std2=0.0),
                 null_images=dict(images=None), null_out=dict(out=None), null_hb=dict(hbounds=None), null_hc=dict(hcoef=None),
                 null_vb=dict(vbounds=None), null_vc=dict(vcoef=None), out_align=dict(out=out.data_ptr() + 4),
                 table_align=dict(vcoef=base[names.index('vcoef')] + 2), hk=dict(hk=0), vk=dict(vk=0), band0=dict(band_rows=0),
                 lds=dict(band_rows=(ops.PIL_LDS_LIMIT - 3072) // (3 * R) + 1), two_gib=dict(B=(1 << 31) // (3 * H * W) + 1), B0=dict(B=0))
    for fn in (lib.sidlsg_pil_patches_u8_f32, lib.sidlsg_pil_patches_u8):
        for what, edit in cases.items():
            assert call(fn, **edit) == EINVAL, what
    assert call(band_rows=(ops.PIL_LDS_LIMIT - 3072) // (3 * R)) == 0, 'the stated limit itself is accepted'
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='multiple of the patch size'):
        ops.pil_patches(img, 30, 8)
    with pytest.raises(RuntimeError, match=r'uint8 \[B, 3, H, W\]'):
        ops.pil_patches(img[:, :2], 32, 8)
    with pytest.raises(RuntimeError, match='uint8'):
        ops.pil_patches(img.float(), 32, 8)
    with pytest.raises(RuntimeError, match='LDS'):
        ops.pil_patches(torch.zeros(1, 3, 4096, 4096, dtype=torch.uint8, device=dev), 224, 14)      # a band of 14 rows reads ~290 source rows


# ---- the tower and the detector ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def detectors(dev, files):
    from sid_lsg_amd.clip import load_open_clip
    return {dt: load_open_clip(files['checkpoint'], files['tokenizer'], dev, arch='tiny', compute_dtype=dt) for dt in (F32, BF16)}


def test_tower_fp32_matches_transformers(dev, ref, detectors):
    """fp32 mode against the golden image_embeds (transformers on the CPU, fed Pillow's pixel_values): the preprocessing is bit-equal,
    so only the reduction order differs.  4x the measured value; the measured value itself must stay under the ceiling."""
    det = detectors[F32]
    assert det.preprocess == 'pil'
    with torch.no_grad():
        emb = det.vision(torch.from_numpy(ref['src/down_40']).to(dev))
    assert emb.dtype == F32 and emb.shape == ref['image_embeds'].shape
    got = F.normalize(emb.cpu().double(), dim=-1)
    want = torch.from_numpy(ref['image_embeds']).double()
    rel = (got - want).norm(dim=-1) / want.norm(dim=-1)
    print(f'tower fp32 (open_clip checkpoint, pil preprocessing): relative l2 per image {rel.tolist()}')
    assert TOWER_F32_REL_L2 <= F32_CEILING
    assert float(rel.max()) <= 4 * TOWER_F32_REL_L2


def test_tower_bf16_cosines(dev, ref, detectors):
    from sid_lsg_amd import ops
    det = detectors[BF16]
    with torch.no_grad():
        emb = det.vision(torch.from_numpy(ref['src/down_40']).to(dev))
        txt = det.text_embeds_from_ids(torch.from_numpy(ref['ids']))
        feats, cos = ops.clip_score(emb, txt.contiguous())
    err = (cos.cpu().double() - torch.from_numpy(ref['cosines']).double()).abs()
    print(f'tower bf16 (open_clip checkpoint, pil preprocessing): |cosine - golden| {err.tolist()}')
    assert float(err.max()) <= 4 * TOWER_BF16_COS
    # the text half is fp32 torch: the bound of the host test
    torch.testing.assert_close(feats[:, feats.shape[1] // 2:].cpu(), torch.from_numpy(ref['text_embeds']), rtol=1e-4, atol=1e-5)


def test_the_two_preprocessings_differ(dev, ref, detectors, files):
    """'interpolate' on the same weights is another picture at 40 -> 32: the selection reaches the kernel."""
    from sid_lsg_amd.clip import load_open_clip
    other = load_open_clip(files['checkpoint'], files['tokenizer'], dev, arch='tiny', compute_dtype=F32, preprocess='interpolate')
    img = torch.from_numpy(ref['src/down_40']).to(dev)
    with torch.no_grad():
        a, b = detectors[F32].vision.embed(img), other.vision.embed(img)
        same = torch.from_numpy(ref['src/same_32']).to(dev)
        assert torch.equal(detectors[F32].vision.embed(same), other.vision.embed(same)), 'at 32 -> 32 neither resamples'
    assert float((a - b).abs().max()) > 1e-2


def test_text_towers_agree(dev, ref, detectors, files):
    """text_tower='hip' against 'torch' on the same checkpoint: the bounds tests/test_gpu_text_hip.py holds for the two."""
    from sid_lsg_amd.clip import load_open_clip
    from sid_lsg_amd.text import HipCLIPTextModel
    hip = load_open_clip(files['checkpoint'], files['tokenizer'], dev, arch='tiny', text_tower='hip')
    assert type(hip.text_encoder) is HipCLIPTextModel
    ids = torch.from_numpy(ref['ids'])
    a = F.normalize(hip.text_embeds_from_ids(ids).cpu().double(), dim=-1)
    b = F.normalize(detectors[BF16].text_embeds_from_ids(ids).cpu().double(), dim=-1)
    want = torch.from_numpy(ref['text_embeds']).double()
    rel = (a - want).norm(dim=-1) / want.norm(dim=-1)
    print(f'HIP text tower: relative l2 per row against the golden text_embeds {rel.tolist()}; against the torch tower '
          f'{((a - b).norm(dim=-1) / b.norm(dim=-1)).tolist()}')
    assert float(rel.max()) <= 4 * TEXT_F32_REL_L2
    assert float(((a - b).norm(dim=-1) / b.norm(dim=-1)).max()) <= 4 * TEXT_F32_REL_L2
    images, texts = torch.from_numpy(ref['src/down_40']).to(dev), ['a cat', 'two dogs on a hill', 'x']
    s, s_torch = hip.scores(images, texts), detectors[BF16].scores(images, texts)
    assert s.shape == (3,) and float((s - s_torch).abs().max()) <= 1e-5


def test_score_is_the_cosine(dev, ref, detectors):
    from sid_lsg_amd import hps
    det = detectors[F32]
    images, texts = torch.from_numpy(ref['src/down_40']).to(dev), ['a cat', 'two dogs on a hill', 'x']
    s = hps.score(det, images, texts)
    f = det(images, texts=texts, div255=True)
    img, txt = f.chunk(2, 1)
    assert s.dtype == F32 and s.shape == (3,) and float((s - (img * txt).sum(-1)).abs().max()) <= 1e-6
    assert float(s.abs().max()) <= 1.0 + 1e-6, 'no logit scale'
    with pytest.raises(ValueError, match='3 images and 2 prompts'):
        hps.score(det, images, texts[:2])


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_generate_hpsv2_end_to_end(dev, files, tmp_path):
    """4 prompts per style at resolution 64 from the seeded tiny teacher: 16 JPEG files and hpsv2.json; the numbers equal hps.score
    run here on the same files; --score_only repeats them exactly."""
    from click.testing import CliRunner
    import generate_hpsv2
    from sid_lsg_amd import hps
    from sid_lsg_amd.clip import load_open_clip
    prompt_dir, prompts = write_prompts(tmp_path / 'prompts', 4)
    out = tmp_path / 'out'
    scorer = ['--outdir', str(out), '--repo_id', 'random:tiny', '--hps_prompts', prompt_dir, '--hps_checkpoint', files['checkpoint'],
              '--hps_tokenizer', files['tokenizer'], '--hps_arch', 'tiny', '--seeds', '0-3', '--batch', '3']
    res = CliRunner().invoke(generate_hpsv2.main, scorer + ['--network', 'teacher', '--teacher_steps', '2', '--guidance_scale', '2',
                                                            '--resolution', '64'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    jpgs = sorted(os.path.relpath(f, out).replace(os.sep, '/') for f in glob.glob(str(out / '*' / '*.jpg')))
    assert jpgs == [f'{s}/{i:05d}.jpg' for s in sorted(STYLES) for i in range(4)]
    with open(out / 'anime' / '00000.jpg', 'rb') as f:
        assert f.read(3) == b'\xff\xd8\xff'
    first = json.load(open(out / 'hpsv2.json'))
    assert 'Average' in res.output and all(s in res.output for s in STYLES)
    det = load_open_clip(files['checkpoint'], files['tokenizer'], dev, arch='tiny')
    mine = {}
    for style in STYLES:
        images = torch.stack([hps.read_image(str(out / style / f'{i:05d}.jpg')) for i in range(4)]).to(dev)
        assert images.shape == (4, 3, 64, 64)
        mine[style] = hps.score(det, images, prompts[style]).cpu().tolist()
    want = hps.aggregate(mine)
    for k, v in want.items():
        assert abs(first[k] - v) <= 1e-6, k
    assert first['num_images'] == {s: 4 for s in STYLES}
    # the same latent for every style: only the prompt differs between <style>/00002.jpg files, so they are different pictures
    a, b = hps.read_image(str(out / 'anime' / '00002.jpg')), hps.read_image(str(out / 'photo' / '00002.jpg'))
    assert not torch.equal(a, b)
    os.replace(out / 'hpsv2.json', out / 'first.json')
    again = CliRunner().invoke(generate_hpsv2.main, scorer + ['--score_only'], catch_exceptions=False)
    assert again.exit_code == 0, again.output
    assert 'Generating' not in again.output
    assert json.load(open(out / 'hpsv2.json')) == first, '--score_only repeats the numbers exactly'


def test_sid_train_reports_hpsv2(dev, files, tmp_path):
    """`sid_train.py --train_mode 0 --network_pkl teacher --metrics hpsv2_test`: one report line with the five keys."""
    from click.testing import CliRunner
    import sid_train
    prompt_dir, _ = write_prompts(tmp_path / 'prompts', 16)
    (tmp_path / 'aesthetics_6_plus.txt').write_text('\n'.join(f'prompt number {i}' for i in range(8)) + '\n')
    runs = tmp_path / 'runs'
    ev = CliRunner().invoke(sid_train.main, [
        '--outdir', str(runs), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny', '--seed', '1', '--resolution', '64',
        '--batch', '8', '--batch-gpu', '8', '--train_mode', '0', '--network_pkl', 'teacher', '--teacher_steps', '2', '--teacher_cfg', '2',
        '--metrics', 'hpsv2_test', '--metric_hps_path', files['checkpoint'], '--hps_prompts', prompt_dir, '--hps_arch', 'tiny',
        '--hps_tokenizer', files['tokenizer']], catch_exceptions=False)
    assert ev.exit_code == 0, ev.output
    run_dir = glob.glob(str(runs / '00000-*'))[0]
    rows = [json.loads(ln) for ln in open(os.path.join(run_dir, 'metric-hpsv2_test.jsonl'))]
    assert len(rows) == 1 and rows[0]['metric'] == 'hpsv2_test'
    r = rows[0]['results']
    assert sorted(r) == sorted(['hpsv2_anime', 'hpsv2_concept-art', 'hpsv2_paintings', 'hpsv2_photo', 'hpsv2'])
    assert all(np.isfinite(v) and abs(v) <= 100 for v in r.values())
    assert abs(r['hpsv2'] - np.mean([r[f'hpsv2_{s}'] for s in STYLES])) <= 1e-9, 'equal counts per style: the average of the four'
