"""The Inception-v3 detector on the GPU (csrc/inception.hip, sid_lsg_amd/inception.py): each kernel against fp64, blocks and the whole
network against the torch.nn restatement of tests/inception_ref.py in fp64, and the metrics that read it end to end.

Bounds.  u = 2^-24.  A convolution output is an fp32 fma chain over K = KH KW Cin products and one add of the bias: every one of
the K + 1 roundings is at most u times a partial sum that sum |x w| + |b| bounds, so |y^ - y| <= (K + 4) u (conv(|x|, |w|) + |b|)
with room for the second-order terms; ReLU is 1-Lipschitz.  The input kernel rounds the weight l once, then a + l (b - a) twice
(b - a is exact for 8-bit values; 2 roundings per lerp) and (t - 128) / 128 (exact for the power of two, 1 rounding in the
subtraction): at most 8 u * 255 / 128 = 9.5e-7; the tests take 2e-6.  Blocks and the network are held to 4 x the error the
restatement itself makes in fp32 on the CPU, measured in the same test."""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R
from test_inception_host import restate_is

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EINVAL = -22


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- convolution --------------------------------------------------------------------------------------------------------------
# (B, H, W, KH, KW, stride, pad_h, pad_w, Cin, Cout)
CONV_CASES = [
    (3, 19, 19, 3, 3, 2, 0, 0, 4, 32),          # the stem: 3 channels and a zero plane
    (2, 5, 6, 1, 7, 1, 0, 3, 128, 192),
    (2, 6, 5, 7, 1, 1, 3, 0, 160, 160),
    (2, 7, 5, 5, 5, 1, 2, 2, 48, 64),
    (2, 9, 9, 3, 3, 2, 0, 0, 288, 384),         # output 4 x 4
    (2, 8, 8, 3, 3, 2, 0, 0, 288, 384),         # output 3 x 3: floor
    (1, 2, 3, 1, 1, 1, 0, 0, 2048, 320),
    (2, 5, 5, 1, 1, 1, 0, 0, 64, 80),
    (2, 7, 7, 3, 3, 1, 0, 0, 80, 192),
    (2, 4, 4, 1, 3, 1, 0, 1, 384, 384),
    (2, 4, 4, 3, 1, 1, 1, 0, 384, 384),
]


def _conv_data(case, seed):
    B, H, W, KH, KW, stride, ph, pw, Cin, Cout = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, KH, KW, Cin, generator=g) / (KH * KW * Cin) ** 0.5
    b = torch.randn(Cout, generator=g)
    if Cin == 4:
        x[..., 3] = 0
        w[..., 3] = 0
    return x, w, b


def _conv_ref(x, w, b, stride, ph, pw):
    """fp64 on the CPU -> (relu(conv + b), the bound's magnitude conv(|x|, |w|) + |b|), both NHWC."""
    xd, wd, bd = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), b.double()
    y = F.conv2d(xd, wd, bd, stride=stride, padding=(ph, pw))
    mag = F.conv2d(xd.abs(), wd.abs(), bd.abs(), stride=stride, padding=(ph, pw))
    return F.relu(y).permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'b{}_{}x{}_k{}x{}_s{}_p{}{}_{}to{}'.format(*c))
def test_conv_against_fp64(case):
    _need_gpu()
    from sid_lsg_amd import ops
    B, H, W, KH, KW, stride, ph, pw, Cin, Cout = case
    x, w, b = _conv_data(case, 17)
    want, mag = _conv_ref(x, w, b, stride, ph, pw)
    got = ops.conv2d_relu_f32(x.cuda(), w.cuda(), b.cuda(), stride=stride, padding=(ph, pw), relu=True).cpu().double()
    assert got.shape == want.shape
    bound = (KH * KW * Cin + 4) * U * mag
    ratio = float(((got - want).abs() / bound).max())
    zeros = float((want == 0).double().mean())
    print(f'conv {case}: max |error| / bound = {ratio:.4f}, {zeros:.0%} of the outputs cut by ReLU')
    assert 0.2 < zeros < 0.8
    assert ratio <= 1.0
    # without ReLU the negative half comes through
    lin = ops.conv2d_relu_f32(x.cuda(), w.cuda(), b.cuda(), stride=stride, padding=(ph, pw), relu=False).cpu().double()
    assert float(lin.min()) < 0 and torch.equal(lin.clamp_min(0), got)


def test_conv_writes_only_its_channel_slice():
    _need_gpu()
    from sid_lsg_amd import ops
    case = (2, 5, 5, 3, 3, 1, 1, 1, 48, 64)
    x, w, b = _conv_data(case, 3)
    out = torch.full((2, 5, 5, 288), -777.25, device='cuda')
    before = _bits(out)
    ret = ops.conv2d_relu_f32(x.cuda(), w.cuda(), b.cuda(), padding=(1, 1), out=out, col=64)
    assert ret is out
    alone = ops.conv2d_relu_f32(x.cuda(), w.cuda(), b.cuda(), padding=(1, 1))
    after = _bits(out)
    assert torch.equal(after[..., :64], before[..., :64]) and torch.equal(after[..., 128:], before[..., 128:])
    assert torch.equal(after[..., 64:128], _bits(alone))
    want, mag = _conv_ref(x, w, b, 1, 1, 1)
    assert float(((alone.cpu().double() - want).abs() / ((9 * 48 + 4) * U * mag)).max()) <= 1.0


def test_conv_refuses_what_it_does_not_support():
    _need_gpu()
    from sid_lsg_amd._lib import lib
    x = torch.zeros(1, 8, 8, 8, device='cuda')
    w = torch.zeros(16 * 7 * 7 * 8, device='cuda')
    y = torch.zeros(1, 8, 8, 16, device='cuda')
    b = torch.zeros(16, device='cuda')
    s = torch.cuda.current_stream().cuda_stream

    def call(ldx=8, ldc=16, Cin=8, Cout=16, KH=3, KW=3, stride=1, ph=1, pw=1, bias=b):
        return lib.sidlsg_conv2d_relu_f32.raw(x.data_ptr(), ldx, w.data_ptr(), y.data_ptr(), ldc, None if bias is None else bias.data_ptr(), 1, 8, 8,
                                              Cin, Cout, KH, KW, stride, ph, pw, 1, s)
    assert call() == 0
    assert call(Cin=6) == EINVAL and call(KH=2) == EINVAL and call(stride=3) == EINVAL
    assert call(KH=7, KW=7, ph=3, pw=3) == EINVAL and call(KH=3, KW=5, pw=2) == EINVAL and call(KH=1, KW=5, ph=0, pw=2) == EINVAL
    assert call(ldx=6) == EINVAL and call(ldc=18) == EINVAL and call(ldc=12) == EINVAL and call(ph=3) == EINVAL and call(bias=None) == EINVAL
    # an operand of 2^31 bytes: 1 x 8 x 8 pixels of 2^23 floats
    assert call(ldx=1 << 23) == EINVAL
    torch.cuda.synchronize()
    assert not y.any()


# ---- pooling ------------------------------------------------------------------------------------------------------------------
def _nchw(x):
    return x.permute(0, 3, 1, 2)


@pytest.mark.parametrize('H,W,k,stride,pad,negative', [(9, 9, 3, 2, 0, False), (8, 8, 3, 2, 0, False), (3, 4, 3, 1, 1, True)])
def test_max_pool_is_bit_equal(H, W, k, stride, pad, negative):
    _need_gpu()
    from sid_lsg_amd import ops
    x = torch.randn(2, H, W, 24, generator=torch.Generator().manual_seed(H * W))
    if negative:
        x = -x.abs() - 0.5              # zero padding would win every border window
    got = ops.pool2d_f32(x.cuda(), k, stride, pad, ops.POOL_MAX).cpu()
    want = F.max_pool2d(_nchw(x), k, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def test_mean_pool_excludes_the_padding():
    _need_gpu()
    from sid_lsg_amd import ops
    x = torch.randn(2, 3, 4, 16, generator=torch.Generator().manual_seed(2))
    got = ops.pool2d_f32(x.cuda(), 3, 1, 1, ops.POOL_MEAN).cpu().double()
    xd = _nchw(x.double())
    want = F.avg_pool2d(xd, 3, stride=1, padding=1, count_include_pad=False).permute(0, 2, 3, 1)
    scale = F.avg_pool2d(xd.abs(), 3, stride=1, padding=1, count_include_pad=False).permute(0, 2, 3, 1)
    ratio = float(((got - want).abs() / (10 * U * scale)).max())
    print(f'mean 3 x 3 / 1 pad 1 at 3 x 4: max |error| / bound = {ratio:.4f}')
    assert ratio <= 1.0
    # a constant image stays constant: corners divide by 4, edges by 6, the two inner pixels of the middle row by 9
    ones = ops.pool2d_f32(torch.full((1, 3, 4, 4), 3.0, device='cuda'), 3, 1, 1, ops.POOL_MEAN).cpu()
    assert torch.equal(ones, torch.full((1, 3, 4, 4), 3.0))
    ramp = torch.arange(12, dtype=torch.float32).reshape(1, 3, 4, 1).repeat(1, 1, 1, 4)
    got = ops.pool2d_f32(ramp.cuda(), 3, 1, 1, ops.POOL_MEAN).cpu()
    assert got[0, 0, 0, 0] == (0 + 1 + 4 + 5) / 4 and got[0, 0, 1, 0] == (0 + 1 + 2 + 4 + 5 + 6) / 6 and got[0, 1, 1, 0] == 5.0


def test_final_mean_pool():
    _need_gpu()
    from sid_lsg_amd import ops
    x = torch.randn(2, 8, 8, 2048, generator=torch.Generator().manual_seed(4))
    got = ops.pool2d_f32(x.cuda(), 8, 8, 0, ops.POOL_MEAN).cpu().double()
    assert got.shape == (2, 1, 1, 2048)
    want = x.double().mean(dim=(1, 2), keepdim=True)
    scale = x.double().abs().mean(dim=(1, 2), keepdim=True)
    ratio = float(((got - want).abs() / (10 * U * scale)).max())
    print(f'8 x 8 mean: max |error| / bound = {ratio:.4f}')
    assert ratio <= 1.0


def test_pool_writes_only_its_channel_slice():
    _need_gpu()
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    x = torch.randn(2, 9, 9, 32, generator=torch.Generator().manual_seed(6)).cuda()
    out = torch.full((2, 4, 4, 96), -777.25, device='cuda')
    before = _bits(out)
    ops.pool2d_f32(x, 3, 2, 0, ops.POOL_MAX, out=out, col=60)
    after = _bits(out)
    assert torch.equal(after[..., :60], before[..., :60]) and torch.equal(after[..., 92:], before[..., 92:])
    assert torch.equal(after[..., 60:92], _bits(ops.pool2d_f32(x, 3, 2, 0, ops.POOL_MAX)))
    s = torch.cuda.current_stream().cuda_stream
    for k, stride, pad, mode, C in ((9, 1, 0, 0, 32), (3, 1, 2, 0, 32), (3, 2, 0, 2, 32), (3, 2, 0, 0, 30), (0, 1, 0, 0, 32)):
        assert lib.sidlsg_pool2d_f32.raw(x.data_ptr(), 32, out.data_ptr(), 96, 2, 9, 9, C, k, stride, pad, mode, s) == EINVAL


# ---- input --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(256, 256), (64, 48), (48, 64), (512, 512), (299, 299)])
def test_input_kernel_against_the_fp64_legacy_tf_resize(H, W):
    _need_gpu()
    from sid_lsg_amd import ops
    img = R.structured_images(2, H, W, seed=H + W)
    got = ops.inception_input_u8(img.cuda()).cpu()
    assert got.shape == (2, 299, 299, 4) and got.dtype == torch.float32
    want = ((R.legacy_tf_resize_299(img) - 128) / 128).permute(0, 2, 3, 1)
    err = float((got[..., :3].double() - want).abs().max())
    print(f'input {H} x {W}: max |error| = {err:.3e} (derived bound 9.5e-7, asserted 2e-6)')
    assert err <= 2e-6
    assert not got[..., 3].any()
    if (H, W) == (299, 299):
        assert torch.equal(got[..., :3], ((img.float() - 128) / 128).permute(0, 2, 3, 1))


# ---- blocks and the whole network ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def nets():
    """The seeded restatement in fp32 and fp64 (CPU) and the HIP detector built from its state dict."""
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    from sid_lsg_amd import inception
    net32 = R.seeded_net(0)
    net64 = R.seeded_net(0).double()
    return net32, net64, inception.HipInceptionV3(net32.state_dict(), 'cuda')


@pytest.mark.parametrize('name,size', [('Mixed_5b', 5), ('Mixed_6a', 9), ('Mixed_7c', 3)])
def test_block_against_fp64(nets, name, size):
    net32, net64, det = nets
    cin = det.widths[name]
    x = F.relu(torch.randn(2, cin, size, size, generator=torch.Generator().manual_seed(size)))      # what a block sees: half zeros
    want = getattr(net64, name)(x.double())
    own = R.rel_l2(getattr(net32, name)(x), want)
    got = det.layer(name, x.permute(0, 2, 3, 1).contiguous().cuda()).permute(0, 3, 1, 2).cpu()
    assert got.shape == want.shape
    err = R.rel_l2(got, want)
    print(f'{name} at {size} x {size}: relative l2 per image {err}, the fp32 restatement {own}, ratio {err / own}')
    assert (err <= 4 * own).all()


@pytest.fixture(scope='module')
def whole(nets):
    """Per input size: the images, the fp64 features and probabilities, the fp32 restatement's error, the HIP results."""
    net32, net64, det = nets
    out = {}
    for H, W in ((256, 256), (64, 48)):
        img = R.structured_images(2, H, W, seed=H)
        f64 = net64(img, return_features=True)
        out[(H, W)] = dict(img=img, f64=f64, own=R.rel_l2(net32(img, return_features=True), f64),
                           p64=net64(img), p64_nobias=net64(img, no_output_bias=True),
                           feat=det(img.cuda(), return_features=True), p=det(img.cuda()), p_nobias=det(img.cuda(), no_output_bias=True))
    return out


@pytest.mark.parametrize('size', [(256, 256), (64, 48)])
def test_network_features_against_fp64(whole, size):
    w = whole[size]
    assert w['feat'].shape == (2, 2048) and w['feat'].dtype == torch.float32
    err = R.rel_l2(w['feat'].cpu(), w['f64'])
    apart = R.rel_l2(w['f64'][:1], w['f64'][1:])
    print(f'network at {size}: relative l2 per image {err}, the fp32 restatement {w["own"]}, ratio {err / w["own"]}; the two images are {apart} apart; '
          f'features mean {float(w["f64"].mean()):.2f} std {float(w["f64"].std()):.2f} zeros {float((w["f64"] == 0).double().mean()):.0%}')
    assert apart[0] > 0.1
    assert (err <= 4 * w['own']).all()


@pytest.mark.parametrize('size', [(256, 256), (64, 48)])
def test_network_probabilities_against_fp64(whole, size):
    w = whole[size]
    for got, want in ((w['p'], w['p64']), (w['p_nobias'], w['p64_nobias'])):
        assert got.shape == (2, 1008)
        err = float((got.cpu().double() - want).abs().max())
        print(f'probabilities at {size}: max |error| = {err:.3e}, largest probability {float(want.max()):.3f}')
        assert err <= 1e-6
    assert float((w['p64'] - w['p64_nobias']).abs().max()) > 1e-4           # the bias matters, so the flag is observable


def test_network_is_batch_invariant_and_repeatable(nets, whole):
    _, _, det = nets
    img = whole[(64, 48)]['img']
    three = torch.cat([img, R.structured_images(1, 64, 48, seed=9)]).cuda()
    batch = det(three, return_features=True)
    again = det(three, return_features=True)
    assert torch.equal(_bits(batch), _bits(again))
    assert batch.data_ptr() != again.data_ptr()                                 # results are fresh tensors, not the kept buffers
    for i in range(3):
        assert torch.equal(_bits(det(three[i:i + 1], return_features=True)), _bits(batch[i:i + 1]))
    assert torch.equal(_bits(batch[:2]), _bits(whole[(64, 48)]['feat']))
    det.max_batch, keep = 2, det.max_batch                                      # a batch above max_batch goes through in chunks
    try:
        assert torch.equal(_bits(det(three, return_features=True)), _bits(batch))
    finally:
        det.max_batch = keep


# ---- end to end ---------------------------------------------------------------------------------------------------------------
class _Images:
    """An in-memory image set with the dataset item contract: uint8 [3, 64, 64] structured images and captions."""
    has_images = True

    def __init__(self, n, seed):
        self.images = list(R.structured_images(n, 64, 64, seed=seed))

    def __len__(self):
        return len(self.images)

    def caption(self, i):
        return f'caption {i}'

    def __getitem__(self, i):
        return self.images[i], self.caption(i)


def _generator(latents, contexts, init_timesteps=None):
    z = F.interpolate(latents[:, :3], size=(64, 64), mode='nearest')
    return torch.tanh(z) * 0.4 + 0.3


def test_metrics_end_to_end(nets, tmp_path):
    net32, _, _ = nets
    from sid_lsg_amd import inception, metrics
    path = str(tmp_path / 'pt_inception.pth')
    torch.save(net32.state_dict(), path)
    det = metrics.load_detector(path, 'cuda')
    assert isinstance(det, inception.HipInceptionV3)
    num_gen = 24
    opts = metrics.MetricOptions(G=_generator, dataset=_Images(12, 5), detector=det, device='cuda', resolution=64, batch_gen=8)
    fid = metrics.compute_fid_and_clip(opts, num_gen)
    kid = metrics.compute_kid(opts, max_real=None, num_gen=num_gen, num_subsets=4, max_subset_size=8)
    mean, std = metrics.compute_is(opts, num_gen, num_splits=3)
    probs = metrics.generator_feature_stats(metrics.is_options(opts), num_gen, capture_all=True)[0].get_all_torch()
    assert probs.shape == (num_gen, 1008) and probs.is_cuda and probs.dtype == torch.float32
    assert float((probs.double().sum(1) - 1).abs().max()) <= 1e-5
    want = restate_is(probs.cpu().numpy(), 3)
    print(f'FID {fid:.6f}, KID {kid:.6e}, IS {mean:.9f} +- {std:.3e}, restatement {want[0]:.9f} +- {want[1]:.3e}')
    assert np.isfinite(fid) and fid > 0 and np.isfinite(kid)
    assert 1.0 <= mean <= 1008 and abs(mean - want[0]) <= 1e-5 * want[0] and abs(std - want[1]) <= 1e-5 * want[0]
    # the features the metric captured are the detector's
    gen = metrics.generator_feature_stats(opts, 8, capture_all=True)[0].get_all_torch()
    assert gen.shape == (8, 2048)


def test_random_detector_is_seeded(capsys):
    _need_gpu()
    from sid_lsg_amd import inception, metrics
    img = R.structured_images(2, 64, 64, seed=21).cuda()
    a = metrics.load_detector('random:inception-v3', 'cuda')
    b = metrics.load_detector('random:inception-v3:0', 'cuda')
    c = metrics.load_detector('random:inception-v3:1', 'cuda')
    assert isinstance(a, inception.HipInceptionV3)
    inception._warned.clear()
    fa, fb, fc = (d(img, return_features=True) for d in (a, b, c))
    assert 'not comparable with published scores' in capsys.readouterr().out
    assert torch.equal(_bits(fa), _bits(fb)) and not torch.equal(fa, fc)
    f = fa.double()
    assert torch.isfinite(f).all() and 0.5 < float(f.mean()) < 10 and float((f == 0).double().mean()) < 0.5      # alive: nothing collapsed


def test_cli_writes_both_metric_lines(tmp_path):
    """sid_train.py --train_mode 0 --network_pkl teacher --metrics is_test,fid_test --metric_pt_path random:inception-v3 on
    random:tiny: one report line each; the real-set statistics of fid_test come from the images of --data, is_test reads neither."""
    _need_gpu()
    import PIL.Image
    from click.testing import CliRunner
    import sid_train
    (tmp_path / 'aesthetics_6_plus.txt').write_text('\n'.join(f'prompt number {i}' for i in range(40)) + '\n')
    data = tmp_path / 'coco'
    data.mkdir()
    rs = np.random.RandomState(11)
    for i in range(5):
        PIL.Image.fromarray(rs.randint(0, 256, (64, 48 if i == 1 else 64, 3)).astype(np.uint8)).save(str(data / f'img_{i}.png'))
        (data / f'img_{i}.txt').write_text(f'evaluation caption {i}\n')
    runs = tmp_path / 'runs'
    ev = CliRunner().invoke(sid_train.main, [
        '--outdir', str(runs), '--data_prompt_text', str(tmp_path), '--data', str(data), '--sd_model', 'random:tiny', '--seed', '1',
        '--resolution', '64', '--batch', '8', '--batch-gpu', '8', '--train_mode', '0', '--network_pkl', 'teacher', '--teacher_steps', '2',
        '--teacher_cfg', '2', '--metrics', 'is_test,fid_test', '--metric_pt_path', 'random:inception-v3'],
        catch_exceptions=False)
    assert ev.exit_code == 0, ev.output
    run_dir = glob.glob(str(runs / '00000-*'))[0]
    isc = [json.loads(ln) for ln in open(os.path.join(run_dir, 'metric-is_test.jsonl'))]
    fid = [json.loads(ln) for ln in open(os.path.join(run_dir, 'metric-fid_test.jsonl'))]
    assert len(isc) == 1 and isc[0]['metric'] == 'is_test' and 1.0 <= isc[0]['results']['is30k_full_mean'] <= 1008
    assert isc[0]['results']['is30k_full_std'] == 0.0                       # one split
    assert len(fid) == 1 and fid[0]['metric'] == 'fid_test' and np.isfinite(fid[0]['results']['fid30k_full'])
    assert json.load(open(os.path.join(run_dir, 'training_options.json')))['metric_pt_path'] == 'random:inception-v3'
