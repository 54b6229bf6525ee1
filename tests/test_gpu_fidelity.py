"""Paired fidelity on the GPU (csrc/fidelity.hip, sid_lsg_amd/fidelity.py): each kernel against fp64 (tests/fidelity_ref.py), LPIPS-VGG
against the torch.nn restatement in fp64, and the two command lines against each other.

Bounds.
  * sidlsg_psnr_ssim_u8: the squared error and the four counts are integers and must be EQUAL to numpy's int64.  ssim_sum: the window
    moments are 121-term fp64 sums of magnitude <= 6.5e4, each carrying about 121 * 2^-53 * 6.5e4 = 1e-9 worst case and 1e-11 typically;
    the variances keep that absolute error, and the formula divides by at least C2 = 58.5 where they matter, so one SSIM term is good
    to well below 1e-9: |ssim_sum - reference| <= 1e-9 ssim_n.
  * sidlsg_lpips_input_u8: bit-equal to the same four fp32 operations in torch on the CPU.
  * sidlsg_lpips_layer_f32: see test_lpips_layer_against_fp64.
  * LPIPS end to end: 4 x the error the fp32 restatement itself makes on the CPU, measured in the same test."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import fidelity_ref as ref
import inception_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
EINVAL = -22


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


# ---- PSNR / SSIM ------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 11, 11), (3, 12, 45), (2, 43, 37), (1, 64, 80)]


def _pair(B, H, W, seed):
    """Random a; b = a plus noise whose amplitude differs per image and per channel (a swapped image or channel changes the answer);
    the LAST image of the batch is identical in a and b (a batch of one has no room for it: its identical pair is a call of its own)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    b = a.copy()
    for i in range(max(B - 1, 1)):
        for c in range(3):
            amp = 2 + 7 * i + 3 * c
            b[i, c] = np.clip(a[i, c].astype(np.int64) + rng.integers(-amp, amp + 1, (H, W)), 0, 255).astype(np.uint8)
    return a, b


def _check_sums(got, want, what):
    """got [B, 8] fp64 (host), want the reference's rows: integers equal, ssim sums within 1e-9 per term.  -> the largest error per term."""
    worst = 0.0
    for i, (g, w) in enumerate(zip(got.tolist(), want)):
        for q in (0, 1, 3, 4, 5, 7):
            assert g[q] == w[q], f'{what}: image {i}, quantity {q}: {g[q]} != {w[q]}'
        for q, n in ((2, w[3]), (6, w[7])):
            err = abs(g[q] - w[q])
            assert err <= 1e-9 * n, f'{what}: image {i}, quantity {q}: |{g[q]} - {w[q]}| = {err} > 1e-9 * {n}'
            if n:
                worst = max(worst, err / n)
    return worst


@pytest.mark.parametrize('B,H,W', SHAPES)
def test_psnr_ssim_against_fp64(dev, B, H, W):
    from sid_lsg_amd import fidelity
    a, b = _pair(B, H, W, seed=H * W)
    want = ref.psnr_ssim_sums(a, b)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    got = fidelity.psnr_ssim_sums(ta, tb).cpu()
    worst = _check_sums(got, want, f'{B} x {H} x {W}')
    print(f'psnr_ssim {B} x {H} x {W}: max |ssim_sum - fp64| / ssim_n = {worst:.3g} (bound 1e-9)')
    # without a mask every position is kept: the _keep outputs are the plain ones bit for bit
    assert torch.equal(got[:, :4], got[:, 4:])
    # the identical pair: exactly
    same = got[B - 1] if B > 1 else fidelity.psnr_ssim_sums(ta, ta).cpu()[0]
    assert same[0] == 0 and same[2] == same[3] and same[3] == 3 * (H - 10) * (W - 10)
    rows = fidelity.psnr_ssim(ta, tb)
    assert (rows[B - 1] if B > 1 else fidelity.psnr_ssim(ta, ta)[0]) == {'mse': 0.0, 'psnr': math.inf, 'ssim': 1.0}
    for i in range(max(B - 1, 1)):
        assert 0 < rows[i]['ssim'] < 1 and rows[i]['mse'] > 0 and rows[i]['psnr'] == pytest.approx(10 * math.log10(65025 / (want[i][0] / want[i][1])), rel=1e-14)
    if B > 2:
        assert rows[0]['mse'] < rows[1]['mse']                     # the amplitudes grow with the image index
    # the same inputs give the same bits
    assert torch.equal(fidelity.psnr_ssim_sums(ta, tb).cpu(), got)
    # a swapped channel changes the answer
    other = fidelity.psnr_ssim_sums(ta, tb[:, [1, 0, 2]].contiguous()).cpu()
    assert other[0, 0] != got[0, 0]


@pytest.mark.parametrize('B,H,W', [(3, 12, 45), (2, 43, 37)])
def test_psnr_ssim_masks(dev, B, H, W):
    from sid_lsg_amd import fidelity
    a, b = _pair(B, H, W, seed=H + W)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    plain = fidelity.psnr_ssim_sums(ta, tb).cpu()
    rng = np.random.default_rng(3)
    random = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    random[0, 0, :4] = (0, 127, 128, 255)                          # both sides of the threshold
    none_in_0 = random.copy()
    none_in_0[0] = 200                                             # nothing kept in image 0
    centre = np.full((B, H, W), 255, np.uint8)
    centre[:, 5, W - 6] = 0                                        # one pixel, a window centre (the last valid column)
    border = np.full((B, H, W), 255, np.uint8)
    border[:, H - 1, 0] = 127                                      # one pixel that is no window centre
    worst = 0.0
    for name, m in (('random', random), ('all kept', np.zeros((B, H, W), np.uint8)), ('nothing kept in image 0', none_in_0),
                    ('one centre pixel', centre), ('one border pixel', border)):
        got = fidelity.psnr_ssim_sums(ta, tb, torch.from_numpy(m).to(dev)).cpu()
        worst = max(worst, _check_sums(got, ref.psnr_ssim_sums(a, b, m), name))
        assert torch.equal(got[:, :4], plain[:, :4]), name         # the mask does not touch the plain figures
        if name == 'all kept':
            assert torch.equal(got[:, 4:], plain[:, :4])
        if name == 'nothing kept in image 0':
            assert got[0, 4:].tolist() == [0, 0, 0, 0]
            row = fidelity.psnr_ssim(ta, tb, torch.from_numpy(m).to(dev))[0]
            assert all(math.isnan(row[k]) for k in fidelity.KEEP_KEYS) and row['ssim'] == float(plain[0, 2]) / float(plain[0, 3])
        if name == 'one centre pixel':
            assert got[:, 5].tolist() == [3] * B and got[:, 7].tolist() == [3] * B
            d = a[:, :, 5, W - 6].astype(np.int64) - b[:, :, 5, W - 6].astype(np.int64)
            assert got[:, 4].tolist() == (d * d).sum(1).tolist()
            assert got[B - 1, 6] == 3.0
        if name == 'one border pixel':
            assert got[:, 5].tolist() == [3] * B and got[:, 7].tolist() == [0] * B and got[:, 6].tolist() == [0] * B
    print(f'psnr_ssim masks {B} x {H} x {W}: max |ssim_sum_keep - fp64| / ssim_n_keep = {worst:.3g} (bound 1e-9)')


def test_psnr_ssim_refusals(dev):
    from sid_lsg_amd import fidelity
    from sid_lsg_amd._lib import lib
    a = torch.zeros(1, 3, 16, 16, dtype=torch.uint8, device=dev)
    out = torch.full((1, 8), -1.0, dtype=torch.float64, device=dev)
    ws = torch.empty(64, dtype=torch.float64, device=dev)
    call = lambda pa, pb, H, W, po, pw: lib.sidlsg_psnr_ssim_u8.raw(pa, pb, None, 1, H, W, po, pw, None)  # noqa: E731
    p, po, pw = a.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert call(p, p, 10, 16, po, pw) == EINVAL and call(p, p, 16, 10, po, pw) == EINVAL
    assert call(None, p, 16, 16, po, pw) == EINVAL and call(p, None, 16, 16, po, pw) == EINVAL
    assert call(p, p, 16, 16, None, pw) == EINVAL and call(p, p, 16, 16, po, None) == EINVAL
    assert call(p, p, 16, 16, po + 4, pw) == EINVAL and call(p, p, 16, 16, po, pw + 4) == EINVAL
    assert lib.sidlsg_psnr_ssim_u8.raw(p, p, None, 0, 16, 16, po, pw, None) == EINVAL
    assert lib.sidlsg_psnr_ssim_u8.raw(p, p, None, 2048, 1024, 1024, po, pw, None) == EINVAL          # 2^31 bytes and more
    assert lib.sidlsg_psnr_ssim_ws_doubles.raw(1, 10, 16) < 0 and lib.sidlsg_psnr_ssim_ws_doubles.raw(2, 17, 33) == 2 * 3 * 2 * 2 * 8
    torch.cuda.synchronize()
    assert bool((out == -1).all())                                 # nothing was launched
    with pytest.raises(RuntimeError, match='11'):
        fidelity.psnr_ssim(a[:, :, :10].contiguous(), a[:, :, :10].contiguous())
    with pytest.raises(RuntimeError, match='mask'):
        fidelity.psnr_ssim(a, a, torch.zeros(1, 16, 15, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError):
        fidelity.psnr_ssim(a.cpu(), a.cpu())


# ---- LPIPS input --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(40, 56), (11, 13)])
def test_lpips_input_bit_equal(dev, H, W):
    from sid_lsg_amd import fidelity
    rng = np.random.default_rng(H)
    a, b = (torch.from_numpy(rng.integers(0, 256, (3, 3, H, W), dtype=np.uint8)) for _ in range(2))
    a[0, :, 0, :4] = torch.tensor([0, 1, 254, 255], dtype=torch.uint8)
    got = fidelity.lpips_input_u8(a.to(dev), b.to(dev)).cpu()
    assert got.shape == (6, H, W, 4) and got.dtype == torch.float32
    shift, scale = torch.tensor(fidelity.SHIFT, dtype=torch.float32), torch.tensor(fidelity.SCALE, dtype=torch.float32)
    x = torch.cat([a, b]).permute(0, 2, 3, 1).float()              # rows 0 .. B-1 from a, then b
    t = x / 127.5
    t = t - 1
    want = (t - shift) / scale
    assert torch.equal(got[..., :3].contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    assert bool((got[..., 3] == 0).all())
    assert not torch.equal(got[:3], got[3:])
    from sid_lsg_amd._lib import lib
    o = torch.empty(6, H, W, 4, device=dev)
    args = (3, H, W, *fidelity.SHIFT, *fidelity.SCALE, None)
    pa = a.to(dev)
    assert lib.sidlsg_lpips_input_u8.raw(None, pa.data_ptr(), o.data_ptr(), *args) == EINVAL
    assert lib.sidlsg_lpips_input_u8.raw(pa.data_ptr(), pa.data_ptr(), o.data_ptr() + 4, *args) == EINVAL
    assert lib.sidlsg_lpips_input_u8.raw(pa.data_ptr(), pa.data_ptr(), o.data_ptr(), 3, H, W, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, None) == EINVAL


# ---- LPIPS layer --------------------------------------------------------------------------------------------------------------------
def _k(C):
    return 2 * (4 * ((C + 63) // 64)) + 18


@pytest.mark.parametrize('C,ldf,h,wd', [(4, 4, 3, 5), (64, 64, 7, 9), (512, 520, 2, 3), (20, 32, 16, 16)])
def test_lpips_layer_against_fp64(dev, C, ldf, h, wd):
    """|got - want| <= k(C) u M, u = 2^-24, M = the pixel mean of sum_c |w_c| (|n0_c| + |n1_c|)^2, n = f / (|f| + 1e-10) in fp64.

    k(C) from the implemented order.  16 lanes share a pixel; a lane owns L = 4 ceil(C / 64) channels at most.  A C-term sum is each
    lane's terms in order (L - 1 adds) and a 4-level butterfly: a term passes through at most L + 3 additions.
      s = sum f^2: one rounding per square, so (L + 4) u relative (all terms are positive);
      n = sqrt(s) + 1e-10: (L + 4) / 2 u from s, + 1 for the root, + 1 for the add;      q = f / n: + 1        -> e_q = (L + 4) / 2 + 3
      d = q0 - q1: e_q (|q0| + |q1|) + 1 |d|                                              -> e_d = e_q + 1, times S = |q0| + |q1|
      d^2: 2 |d| e_d S + 1 d^2 <= (2 e_d + 1) S^2;   w d^2: + 1;   the weighted sum: + L + 3
    together 2 ((L + 4) / 2 + 4) + 2 + L + 3 = 2 L + 17, and 1 for the second-order terms: k(C) = 2 L + 18 (26 for C <= 64, 82 for
    C = 512).  The double accumulation over the pixels and the division by their count round at 2^-53."""
    from sid_lsg_amd import fidelity
    B = 3
    g = torch.Generator().manual_seed(C + h)
    F = torch.randn(2 * B, h, wd, ldf, generator=g) * torch.tensor([0.3, 1.0, 40.0, 2.0, 1.0, 0.01])[:, None, None, None]
    F[B + 1] = F[1]                                                # image 1: identical halves
    zero = torch.rand(2 * B, h, wd, generator=g) < 0.25            # all-zero pixels (after a ReLU): in one half, the other, or both
    zero[B + 1] = zero[1]
    F[zero] = 0.0
    F[0, 0, 0], F[B, 0, 0] = 0.0, 0.0                              # zero in both halves of a pair that differs elsewhere
    if ldf > C:
        F[..., C:] = float('nan')                                  # the columns past C are not read
    w = torch.rand(C, generator=g) * 0.1
    want, M = ref.lpips_layer(F, w, C)
    got = fidelity.lpips_layer_f32(F.to(dev), w.to(dev)).cpu()
    assert got.dtype == torch.float64 and got.shape == (B,) and bool(torch.isfinite(got).all())
    assert got[1] == 0.0
    ratio = (got - want).abs() / (_k(C) * U * M)
    print(f'lpips_layer C {C} ldf {ldf} {h} x {wd}: values {want.tolist()}, error / bound {ratio.tolist()} (k = {_k(C)})')
    assert bool((want[[0, 2]] > 0).all()) and bool((ratio <= 1).all())
    assert torch.equal(fidelity.lpips_layer_f32(F.to(dev), w.to(dev)).cpu(), got)


def test_lpips_layer_refusals(dev):
    from sid_lsg_amd._lib import lib
    F = torch.zeros(2, 2, 2, 8, device=dev)
    w = torch.zeros(8, device=dev)
    out = torch.full((1,), -1.0, dtype=torch.float64, device=dev)
    ws = torch.empty(8, dtype=torch.float64, device=dev)
    call = lambda pf, ldf, pw, C, po, pws: lib.sidlsg_lpips_layer_f32.raw(pf, ldf, pw, 1, 2, 2, C, po, pws, None)  # noqa: E731
    pf, pw, po, pws = F.data_ptr(), w.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert call(pf, 8, pw, 6, po, pws) == EINVAL and call(pf, 6, pw, 4, po, pws) == EINVAL and call(pf, 4, pw, 8, po, pws) == EINVAL
    assert call(None, 8, pw, 8, po, pws) == EINVAL and call(pf, 8, None, 8, po, pws) == EINVAL
    assert call(pf, 8, pw, 8, None, pws) == EINVAL and call(pf, 8, pw, 8, po, None) == EINVAL
    assert call(pf + 4, 8, pw, 8, po, pws) == EINVAL and call(pf, 8, pw, 0, po, pws) == EINVAL
    assert lib.sidlsg_lpips_layer_ws_doubles.raw(0, 2, 2) < 0 and lib.sidlsg_lpips_layer_ws_doubles.raw(3, 16, 17) == 3 * 3
    torch.cuda.synchronize()
    assert float(out[0]) == -1.0


# ---- LPIPS end to end -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lpips_nets(dev):
    """The seeded restatement in fp32 and fp64 (CPU) and HipLPIPS, all three from the same two state dicts."""
    from sid_lsg_amd import fidelity
    vgg, lin = fidelity.random_state_dicts(0)
    return ref.LpipsVgg().load(vgg, lin).eval(), ref.LpipsVgg().load(vgg, lin).double().eval(), fidelity.load_lpips('random:lpips-vgg', 'random:lpips-vgg', dev)


def _count_launches(monkeypatch, fn):
    """fn() with every entry point of the library counted -> (result, {name: calls})."""
    from sid_lsg_amd._lib import lib
    counts = {}
    for name in lib.protos:
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*a)
        counted.raw = real.raw
        monkeypatch.setitem(lib.__dict__, name, counted)
    out = fn()
    monkeypatch.undo()
    return out, counts


@pytest.mark.parametrize('H,W', [(40, 56), (32, 32)])
def test_lpips_against_fp64(dev, lpips_nets, monkeypatch, H, W):
    """B = 2 pairs.  The features at every tap and the five per-tap distances of a pair are held to 4 x the error of the fp32
    restatement on the CPU (relative l2 per image, test_gpu_inception.py's measure: over a tap's feature map, and over the vector of
    the five per-tap distances -- the LPIPS value itself is their sum, a single number whose signed errors can cancel to nothing in
    either run, so its own error is printed and not divided)."""
    net32, net64, hip = lpips_nets
    a = inception_ref.structured_images(2, H, W, seed=H)
    b = inception_ref.structured_images(2, H, W, seed=H + 1)
    with torch.no_grad():
        want = net64.tap_values(a, b)                             # [5, 2]
        cpu = net32.tap_values(a, b)
        f64, f32 = net64.taps(torch.cat([a, b])), net32.taps(torch.cat([a, b]))
    (got, feats), counts = _count_launches(monkeypatch, lambda: (hip.tap_values(a.to(dev), b.to(dev)).cpu().clone(),
                                                                 [f.permute(0, 3, 1, 2).cpu() for f in hip.taps(a.to(dev), b.to(dev))]))
    # one tap_values pass and one taps pass: 2 x (1 input + 13 convolutions + 4 pools) and 5 layer launches
    assert counts == {'sidlsg_lpips_input_u8': 2, 'sidlsg_conv2d_relu_f32': 26, 'sidlsg_pool2d_f32': 8, 'sidlsg_lpips_layer_f32': 5}, counts
    _, counts = _count_launches(monkeypatch, lambda: hip(a.to(dev), b.to(dev)))
    assert sum(counts.values()) == 13 + 4 + 5 + 1 + 1 and counts['sidlsg_lpips_layer_f32'] == 5 and counts['sidlsg_lpips_sum_f64'] == 1, counts     # + the final add
    for i, (f, w64, w32) in enumerate(zip(feats, f64, f32)):
        assert f.shape == w64.shape and bool(torch.isfinite(f).all()) and bool((f != 0).any()), f'tap {i}'
        alive = float((w64 > 0).double().mean())
        err, own = inception_ref.rel_l2(f, w64), inception_ref.rel_l2(w32, w64)
        print(f'LPIPS {H} x {W} tap {i} {tuple(f.shape[1:])}: {alive:.0%} of the features alive; relative l2 per image {err}, the fp32 restatement {own}, ratio {err / own}')
        assert alive > 0.05 and (err <= 4 * own).all()
    err, own = inception_ref.rel_l2(got.T, want.T), inception_ref.rel_l2(cpu.T, want.T)
    total = hip(a.to(dev), b.to(dev)).cpu()
    assert torch.equal(total, (((got[0] + got[1]) + got[2]) + got[3]) + got[4])          # the taps in order
    print(f'LPIPS {H} x {W}: values {want.sum(0).tolist()}; per-tap vector, relative l2 per image {err}, the fp32 restatement {own}, ratio {err / own}; '
          f'|LPIPS - fp64| {(total - want.sum(0)).abs().tolist()}, the fp32 restatement {(cpu.double().sum(0) - want.sum(0)).abs().tolist()}')
    assert bool((want.sum(0) > 1e-3).all()) and (err <= 4 * own).all()
    # identical pairs: exactly 0, also as one pair of a batch whose other pair differs
    assert hip(a.to(dev), a.to(dev)).tolist() == [0.0, 0.0]
    mixed = hip(torch.stack([a[0], a[1]]).to(dev), torch.stack([a[0], b[1]]).to(dev)).tolist()
    assert mixed[0] == 0.0 and mixed[1] == float(total[1])


def test_lpips_chunks_and_refusals(dev, lpips_nets):
    from sid_lsg_amd import fidelity
    hip = lpips_nets[2]
    assert fidelity.HipLPIPS.max_pairs(512, 512) == 8 and fidelity.HipLPIPS.max_pairs(1024, 1024) == 2 and fidelity.HipLPIPS.max_pairs(64, 64) == 512
    assert 2 * 8 * 512 * 512 * 64 * 4 < 2 ** 31                   # the first stage's map of 8 pairs
    a = inception_ref.structured_images(3, 16, 24, seed=1).to(dev)
    b = inception_ref.structured_images(3, 16, 24, seed=2).to(dev)
    whole = hip(a, b)
    parts = torch.cat([hip(a[:2], b[:2]), hip(a[2:], b[2:])])
    assert torch.equal(whole, parts)                               # a pair does not depend on the batch it travels in
    with pytest.raises(ValueError, match='too small'):
        hip(a[:, :, :12, :12].contiguous(), b[:, :, :12, :12].contiguous())
    with pytest.raises(RuntimeError):
        hip(a, b[:, :, :8].contiguous())


# ---- command lines ----------------------------------------------------------------------------------------------------------------------
def test_generate_onestep_fidelity_equals_the_tool(dev, tmp_path):
    """--fidelity 1 with --init_images, --mask_images, --mask_composite 1 and random LPIPS specs writes fidelity.json whose per-image
    figures are those tools/image_pair_fidelity.py computes from the written PNG files; the composited kept region is the init
    image's bits (mse_keep 0, psnr_keep inf) while the whole image is not.  ssim_keep counts the windows whose CENTRE is kept, and a
    window centred within 5 pixels of the repainted region covers repainted pixels: under the run's own mask ssim_keep is the fp64
    reference's value, above the whole image's and below 1.  It is exactly 1 over the windows that see composited pixels only, which
    the tool is asked for with the mask's repainted region grown by 5 pixels."""
    import PIL.Image
    from click.testing import CliRunner
    import generate_onestep
    spec = importlib.util.spec_from_file_location('image_pair_fidelity', os.path.join(ROOT, 'tools', 'image_pair_fidelity.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    prompts = tmp_path / 'prompts.txt'
    prompts.write_text('a red cube\na blue sphere\n')
    D, M = tmp_path / 'init', tmp_path / 'masks'
    D.mkdir()
    M.mkdir()
    init = inception_ref.structured_images(2, 64, 64, seed=4).permute(0, 2, 3, 1).numpy()
    for i in range(2):
        PIL.Image.fromarray(np.ascontiguousarray(init[i]), 'RGB').save(D / f'{i}.png')     # already 64 x 64: the crop is the file
    mask = np.zeros((64, 64), np.uint8)
    mask[8:40, 24:64] = 255
    mask[50, 3] = 127
    PIL.Image.fromarray(mask, 'L').save(M / 'm.png')
    out = tmp_path / 'out'
    lp = ['--lpips_vgg', 'random:lpips-vgg:1', '--lpips_lin', 'random:lpips-vgg:1']
    r = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out), '--network', 'teacher', '--repo_id', 'random:tiny', '--teacher_steps', '2',
                                                   '--guidance_scale', '2', '--init_images', str(D), '--mask_images', str(M), '--strength', '1',
                                                   '--mask_composite', '1', '--resolution', '64', '--seeds', '0-2', '--batch', '2',
                                                   '--text_prompts', str(prompts), '--fidelity', '1', *lp], catch_exceptions=False)
    assert r.exit_code == 0, r.output
    assert 'Fidelity over 3 images' in r.output and 'not comparable' in r.output
    with open(out / 'fidelity.json') as f:
        report = json.load(f)
    assert sorted(report) == ['mean', 'options', 'per_image'] and sorted(report['per_image']) == ['000000.png', '000001.png', '000002.png']
    assert report['options']['init_images'] == str(D) and report['options']['mask_composite'] is True and report['options']['lpips_vgg'] == 'random:lpips-vgg:1'
    for row in report['per_image'].values():
        assert sorted(row) == sorted(('mse', 'psnr', 'ssim', 'mse_keep', 'psnr_keep', 'ssim_keep', 'lpips'))
        assert row['psnr_keep'] == math.inf and row['mse_keep'] == 0
        assert math.isfinite(row['psnr']) and 0 < row['ssim'] < row['ssim_keep'] < 1 and row['lpips'] > 0
    for key, name in ((0, '000000.png'), (1, '000001.png'), (2, '000002.png')):          # sample 2 started from init file 2 mod 2 = 0
        png = np.asarray(PIL.Image.open(out / name).convert('RGB')).transpose(2, 0, 1)[None]
        want = ref.psnr_ssim_sums(png, init[key % 2].transpose(2, 0, 1)[None], mask[None])[0]
        row = report['per_image'][name]
        assert row['mse'] == want[0] / want[1] and abs(row['ssim'] - want[2] / want[3]) <= 1e-9 and abs(row['ssim_keep'] - want[6] / want[7]) <= 1e-9
    mean = report['mean']
    assert mean['psnr_keep'] == math.inf and mean['mse_keep'] == 0 and math.isfinite(mean['psnr'])
    assert mean['lpips'] == pytest.approx(sum(r_['lpips'] for r_ in report['per_image'].values()) / 3, rel=1e-15)
    # the stand-alone tool on the written files: sample 2 pairs with init file 2 mod 2 = 0
    r = CliRunner().invoke(tool.main, ['--ref', str(D), '--test', str(out), '--masks', str(M), '--batch', '2', *lp], catch_exceptions=False)
    assert r.exit_code == 0, r.output
    again = json.loads(r.output[r.output.index('{'):])
    assert again['per_image'] == report['per_image'] and again['mean'] == report['mean']
    # the windows that see composited pixels only: the repainted region grown by the window's radius
    from scipy.ndimage import maximum_filter
    G = tmp_path / 'grown'
    G.mkdir()
    grown = maximum_filter(mask, size=11, mode='constant', cval=0)
    assert 0 < int((grown[5:-5, 5:-5] < 128).sum()) < int((mask[5:-5, 5:-5] < 128).sum())
    PIL.Image.fromarray(grown, 'L').save(G / 'm.png')
    r = CliRunner().invoke(tool.main, ['--ref', str(D), '--test', str(out), '--masks', str(G)], catch_exceptions=False)
    assert r.exit_code == 0, r.output
    inner = json.loads(r.output[r.output.index('{'):])
    for name, row in inner['per_image'].items():
        assert row['ssim_keep'] == 1.0 and row['psnr_keep'] == math.inf and row['ssim'] == report['per_image'][name]['ssim']
    assert inner['mean']['ssim_keep'] == 1.0
    # without the LPIPS specs: the same PSNR / SSIM figures and no lpips key
    r = CliRunner().invoke(tool.main, ['--ref', str(D), '--test', str(out), '--batch', '3'], catch_exceptions=False)
    assert r.exit_code == 0, r.output
    plain = json.loads(r.output[r.output.index('{'):])
    for name, row in plain['per_image'].items():
        assert sorted(row) == ['mse', 'psnr', 'ssim'] and all(row[k] == report['per_image'][name][k] for k in row)
