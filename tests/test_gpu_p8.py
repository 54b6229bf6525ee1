"""The 256-row-tile GEMM / conv3x3 kernels (csrc/gemm_p8.h): both configurations forced on (sidlsg_debug_set_p8) against
  (a) fp32 PyTorch references on the CPU (the bar of tests/test_gpu_ops.py),
  (b) gemm_v3_kernel BIT FOR BIT wherever neither side splits K (same K order and MFMA operand placement by construction),
over: every epilogue feature set (bias / + residual / + time-embedding row vector / both / SiLU / fp32 output / fp32 accumulate),
ragged row counts (tiles with out-of-range rows), grouped launches (two weight sets, `_g2`), split-K slabs, stride-2 convs,
tiles spanning several images (8 x 8 latents: 4 images per 256-row tile), and repeated launches (race screen of the counted-wait
pipeline: the result of 20 launches must not move).  Shapes are the UNet's own."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


@pytest.fixture()
def p8(dev):
    """p8.set(mode): -1 rule, 0 never (v3), 1 / 2 = S / W forced; restored afterwards."""
    from sid_lsg_amd._lib import lib

    class Ctl:
        def set(self, mode):
            lib.sidlsg_debug_set_p8.raw(mode)
    old = lib.sidlsg_debug_set_p8.raw(-1)
    yield Ctl()
    lib.sidlsg_debug_set_p8.raw(old)


def rnd(*shape, seed=0, scale=1.0, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def close(got, ref, tol, what):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert torch.isfinite(got).all(), what
    err = ((got - ref).abs().max() / (ref.abs().max() + 1e-12)).item()
    assert err < tol, f'{what}: rel max err {err:.3e} (tol {tol})'


def conv_ref(x, w, stride):
    B, H, W, Cin = x.shape
    wt = w.float().view(-1, 3, 3, Cin).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), wt, stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


# (B, H, Cin, Cout, stride): W takes Cout % 320 == 0, S Cout % 160 == 0; 8 x 8 x B16: four images per tile; B3: ragged tiles.
# The other side (p8 off), by the dispatch record: gemm_bf16_kernel<64, 64, 1> for all but (2, 16, 320, 960) -- gemm_v3_kernel<1> with 5 K splits,
# against 3 splits of either forced p8 configuration -- and the last two
CONV = [(4, 32, 64, 320, 1), (3, 32, 128, 320, 1), (16, 8, 128, 640, 1), (4, 32, 64, 320, 2), (2, 16, 320, 960, 1), (5, 8, 64, 160, 1),
        (16, 32, 128, 320, 1), (17, 32, 64, 640, 1)]          # the last two: >= 256 tiles of 128 x 160 -> the other side IS gemm_v3_kernel, unsplit


def v3_runs_unsplit(M, N, K):
    """dispatch_gemm takes gemm_v3_kernel without split-K (the kernel the p8 kernels are bit-identical to): N % 160 == 0 and >= 256 tiles
    of 128 x 160; smaller launches run gemm_bf16_kernel, whose conv K order is tap-major."""
    return N % 160 == 0 and ((M + 127) // 128) * (N // 160) >= 256


def p8_runs_unsplit(mode, M, N, K):
    """The FORCED p8 configurations split K towards one block per CU (gemm.hip::dispatch_gemm: fewer than 192 tiles of 256 x 320 / 256 x 160
    and at least 24 K-tiles): a split launch sums its slabs in another order than gemm_v3_kernel's single accumulation chain."""
    return ((M + 255) // 256) * (N // (320 if mode == 2 else 160)) >= 192 or (K // 64) // 12 < 2


@pytest.mark.parametrize('B,H,Cin,Cout,stride', CONV)
@pytest.mark.parametrize('mode', [1, 2])
def test_conv_forced(dev, p8, mode, B, H, Cin, Cout, stride):
    from sid_lsg_amd import ops
    if Cout % (320 if mode == 2 else 160):
        pytest.skip('configuration does not take this channel count')
    x, w = rnd(B, H, H, Cin, seed=1), rnd(Cout, 9 * Cin, seed=2, scale=(9 * Cin) ** -0.5)
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(3))
    rv = torch.randn(B, Cout, generator=torch.Generator().manual_seed(5))
    ref = conv_ref(x, w, stride)
    res = rnd(*ref.shape, seed=6)
    xd, wd, bd, rd, rvd = x.to(dev), w.to(dev), bias.to(dev), res.to(dev), rv.to(dev)
    cases = dict(plain={}, bias=dict(bias=bd), res=dict(bias=bd, res=rd), rowvec=dict(bias=bd, rowvec=rvd), both=dict(bias=bd, res=rd, rowvec=rvd),
                 f32=dict(bias=bd, res=rd, out_f32=True))
    for name, kw in cases.items():
        p8.set(0)
        y3 = ops.conv3x3(xd, wd, stride=stride, **kw)
        p8.set(mode)
        y8 = ops.conv3x3(xd, wd, stride=stride, **kw)
        r = ref + (bias if 'bias' in kw else 0) + (res.float() if 'res' in kw else 0) + (rv[:, None, None, :] if 'rowvec' in kw else 0)
        close(y8, r, 2e-3 if kw.get('out_f32') else 1.2e-2, f'conv {name}')
        if v3_runs_unsplit(ref.shape[0] * ref.shape[1] * ref.shape[2], Cout, 9 * Cin) and p8_runs_unsplit(mode, ref.shape[0] * ref.shape[1] * ref.shape[2], Cout, 9 * Cin):
            assert torch.equal(y8, y3), f'conv {name}: not bit-identical to gemm_v3_kernel'
    # race screen: 20 launches, one answer
    p8.set(mode)
    y0 = ops.conv3x3(xd, wd, bias=bd, res=rd, stride=stride)
    for _ in range(20):
        assert torch.equal(ops.conv3x3(xd, wd, bias=bd, res=rd, stride=stride), y0)


# The other side (p8 off), by the dispatch record: gemm_bf16_kernel<64, 64> for (4096, 320, 320), (1000, 320, 640), (300, 960, 1280) and
# (20000, 160, 320); gemm_v3_kernel with 2 / 4 K splits for (8192, 640, 2560) / (2048, 1280, 5120) (forced p8: 2 / 4 splits on S, 3 / 6 on W);
# unsplit gemm_v3_kernel for the last two
@pytest.mark.parametrize('M,N,K', [(4096, 320, 320), (1000, 320, 640), (8192, 640, 2560), (300, 960, 1280), (20000, 160, 320), (2048, 1280, 5120),
                                   (16500, 320, 640), (8192, 640, 1280)])
@pytest.mark.parametrize('mode', [1, 2])
def test_gemm_forced(dev, p8, mode, M, N, K):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    from sid_lsg_amd.ops import _p, _s
    if N % (320 if mode == 2 else 160):
        pytest.skip('configuration does not take this width')
    ops.ensure_workspace(dev)
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3))
    res = rnd(M, N, seed=4)
    ref = a.float() @ w.float().t()
    ad, wd, bd, rd = a.to(dev), w.to(dev), bias.to(dev), res.to(dev)
    for name, kw, r in (('plain', {}, ref), ('bias+res', dict(bias=bd, res=rd), ref + bias + res.float()), ('f32', dict(bias=bd, out_f32=True), ref + bias)):
        p8.set(0)
        y3 = ops.gemm(ad, wd, **kw)
        p8.set(mode)
        y8 = ops.gemm(ad, wd, **kw)
        close(y8, r, 2e-3 if kw.get('out_f32') else 1.2e-2, f'gemm {name}')
        if v3_runs_unsplit(M, N, K) and p8_runs_unsplit(mode, M, N, K):
            assert torch.equal(y8, y3), f'gemm {name}: not bit-identical to gemm_v3_kernel'
    # SiLU and fp32 accumulate through the raw entry point (flags 2 / 1 | 4)
    p8.set(mode)
    y = torch.empty(M, N, device=dev, dtype=BF16)
    lib.sidlsg_gemm_bf16(_p(ad), K, _p(wd), _p(y), N, _p(bd), None, 0, None, 0, 1, M, N, K, 1.0, 2, _s())
    close(y, torch.nn.functional.silu(ref + bias), 1.2e-2, 'gemm SiLU')
    acc = torch.full((M, N), 0.5, device=dev, dtype=F32)
    lib.sidlsg_gemm_bf16(_p(ad), K, _p(wd), _p(acc), N, None, None, 0, None, 0, 1, M, N, K, 1.0, 1 | 4, _s())
    close(acc - 0.5, ref, 2e-3, 'gemm fp32 accumulate')


@pytest.mark.parametrize('mode', [1, 2])
def test_grouped_conv_forced(dev, p8, mode):
    """Two weight sets on one stacked batch (the frozen pair pass): each half equals the single-set launch of its own weights, bit for bit;
    an odd number of 256-row tiles per set (B 6 x 16 x 16 = 768 rows per set)."""
    from sid_lsg_amd import ops
    B, H, Cin, Cout = 6, 16, 128, 320
    x = rnd(B, H, H, Cin, seed=1).to(dev)
    w0, w1 = rnd(Cout, 9 * Cin, seed=2, scale=0.03).to(dev), rnd(Cout, 9 * Cin, seed=3, scale=0.03).to(dev)
    b0, b1 = torch.randn(Cout, device=dev), torch.randn(Cout, device=dev)
    res = rnd(B, H, H, Cout, seed=4).to(dev)
    p8.set(mode)
    y = ops.conv3x3(x, ops.Pair(w0, w1), bias=ops.Pair(b0, b1), res=res)
    ya = ops.conv3x3(x[:B // 2].contiguous(), w0, bias=b0, res=res[:B // 2].contiguous())
    yb = ops.conv3x3(x[B // 2:].contiguous(), w1, bias=b1, res=res[B // 2:].contiguous())
    assert torch.equal(y[:B // 2], ya) and torch.equal(y[B // 2:], yb)
    p8.set(0)      # 12 tiles of 128 x 160: dispatch_gemm takes gemm_bf16_kernel here (tap-major K order), so equal up to the summation order only
    close(ops.conv3x3(x, ops.Pair(w0, w1), bias=ops.Pair(b0, b1), res=res), y, 1.2e-2, 'grouped conv: p8 vs the default kernels')


def _last_kernel():
    """(kernel, tile rows, tile columns, K splits) of the dispatch record (include/sidlsg_hip.h sidlsg_debug_last_launch)."""
    import ctypes
    from sid_lsg_amd._lib import lib
    r = (ctypes.c_int * 10)()
    assert lib.sidlsg_debug_last_launch.raw(ctypes.addressof(r), 10) == 10
    return r[0], r[1], r[2], r[6]


def test_rule_takes_the_wide_tile_for_the_big_convs(dev, p8):
    """The dispatch rule (cost model in gemm.hip::p8_rule): B16 64x64 320->320 goes to the 256 x 320 kernel (bit-identical to v3 there),
    a B2 call of the same layer does not fill 256-row tiles and stays on v3 (with 4 K splits).  The dispatch record names the kernel of
    each call: SIDLSG_K_GEMM_V3 = 2, SIDLSG_K_GEMM_P8W = 4."""
    from sid_lsg_amd import ops
    V3, P8W = 2, 4
    x, w = rnd(16, 64, 64, 320, seed=1).to(dev), rnd(320, 2880, seed=2, scale=0.02).to(dev)
    p8.set(-1)
    y = ops.conv3x3(x, w)
    assert _last_kernel() == (P8W, 256, 320, 1), _last_kernel()
    y2 = ops.conv3x3(x[:2].contiguous(), w)
    assert _last_kernel() == (V3, 128, 160, 4), _last_kernel()
    p8.set(0)
    assert torch.equal(ops.conv3x3(x, w), y)
    assert _last_kernel() == (V3, 128, 160, 1), _last_kernel()
    assert torch.equal(ops.conv3x3(x[:2].contiguous(), w), y2)
    assert _last_kernel() == (V3, 128, 160, 4), _last_kernel()
