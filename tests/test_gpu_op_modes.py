"""The modes of the weight-bearing autograd nodes (ops._Linear, _Conv3x3, _GroupNorm, _LayerNorm, _NormLinear, _NormConv): one node
per op, in its single form with tensor parameters and in its grouped form with ops.Pairs (dual_networks).  The numerical contract of
the kernels and of the networks is held by test_gpu_ops / test_gpu_grouped / test_gpu_grouped_fp8; what is pinned here, at the op
level, is what a fold of the two forms can get wrong:
  * routing: every gradient slot (x, res, rowvec) of the grouped form against two single frozen calls on the halves;
  * the row-vector gradient of the single e4m3 conv node;
  * retention: which tensors the grouped form keeps alive for its backward;
  * the two-launch fallback of the grouped LayerNorm for halves of no multiple of 16 rows, forward and backward."""
import contextlib

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


def rnd(*shape, seed=0, scale=1.0, dev=None):
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(*shape, generator=g) * scale).to(BF16)
    return t.to(dev) if dev is not None else t


def P(t):
    return torch.nn.Parameter(t, requires_grad=False)


def same_or_close(got, ref, what):      # the rule of tests/test_gpu_grouped.py
    if torch.equal(got, ref):
        return 'bit-equal'
    err = float((got.float() - ref.float()).abs().max() / (ref.float().abs().max() + 1e-12))
    assert err < 1e-2, f'{what}: grouped node differs from the two single calls by {err:.3g} of max'
    return f'within {err:.1e}'


def two_sets(dev, C, N, conv=False, e4m3=False):
    """Two frozen parameter sets of one layer (norm scale / shift, master weight, bias, forward copy, backward-data operand) and the
    partner map that dual_networks takes."""
    from sid_lsg_amd import ops
    sets = []
    for s0 in (10, 20):
        K = 9 * C if conv else C
        w = rnd(N, K, seed=s0, scale=K ** -0.5, dev=dev)
        wt = ops.transpose_w(w.float().view(N, 9, C), N, C, 9) if conv else w.t().contiguous()
        master = w.float().view(N, 9, C).permute(0, 2, 1).reshape(N, C, 3, 3).contiguous() if conv else w.float()
        sets.append(dict(gamma=P(rnd(C, seed=s0 + 1, dev=dev).float() + 1.0), beta=P(rnd(C, seed=s0 + 2, dev=dev).float()), weight=P(master),
                         bias=P(rnd(N, seed=s0 + 3, dev=dev).float()), w16=ops.Fp8Weight(w) if e4m3 else w, w16t=wt))
    a, b = sets
    return a, b, {id(a[k]): b[k] for k in a}


def weight_shapes(st):
    w = st['w16']
    return {tuple(st['weight'].shape), tuple(w.shape), tuple(st['w16t'].shape)}


def dual(pmap, on=True):
    from sid_lsg_amd import ops
    return ops.dual_networks(pmap) if on else contextlib.nullcontext()


# ------------------------------------------------------------------------------------------------------------------ routing
def _route(run, n, dy):
    """run(rows, set, grouped) -> (y, dx, dres, drowvec) for the samples / row blocks `rows` of the stacked batch of n."""
    a, b = run.sets
    y, dx, dres, drv = run(slice(0, 2 * n), a, True)
    parts = [run(slice(0, n), a, False), run(slice(n, 2 * n), b, False)]
    how = [same_or_close(got, torch.cat([p[i] for p in parts]), what) for i, got, what in ((0, y, 'output'), (1, dx, 'dx'), (3, drv, 'drowvec'))]
    assert torch.equal(dres, dy), 'the residual gradient is the incoming gradient'
    assert not torch.equal(y[y.shape[0] // 2:], run(slice(n, 2 * n), a, False)[0]), 'the second half must have used the second set'
    return how


def test_linear_routes_gradients_in_the_grouped_form(dev):
    """2 x 64 rows, K = 64, N = 160 (the 160-wide tile path), a row vector per 16 rows."""
    from sid_lsg_amd import ops
    Mh, K, N, rpb = 64, 64, 160, 16
    a, b, pmap = two_sets(dev, K, N)
    x, res, dy = rnd(2 * Mh, K, seed=1, dev=dev), rnd(2 * Mh, N, seed=2, dev=dev), rnd(2 * Mh, N, seed=3, dev=dev)
    rv = rnd(2 * Mh // rpb, N, seed=4, dev=dev).float()

    def run(rows, st, grouped):
        xg, rg = x[rows].clone().requires_grad_(), res[rows].clone().requires_grad_()
        vg = rv[rows.start // rpb:rows.stop // rpb].clone().requires_grad_()
        with dual(pmap, grouped):
            y = ops.linear(xg, st['weight'], st['bias'], st['w16'], st['w16t'], res=rg, rowvec=vg, rows_per_batch=rpb)
        y.backward(dy[rows])
        return y.detach(), xg.grad, rg.grad, vg.grad
    run.sets = (a, b)
    print(f'linear 2x{Mh} x {N} x {K}: y / dx / drowvec {_route(run, Mh, dy)}')


@pytest.mark.parametrize('stride,ups', [(1, 0), (2, 0), (1, 1)])
def test_conv3x3_routes_gradients_in_the_grouped_form(dev, stride, ups):
    """2 samples, 8 x 8 (from 4 x 4 with the fused upsample), 64 -> 160 channels: one variant per branch of the data gradient."""
    from sid_lsg_amd import ops
    Bh, H, W, Cin, Cout = 1, 8, 8, 64, 160
    a, b, pmap = two_sets(dev, Cin, Cout, conv=True)
    Hs, Ws = (H // 2, W // 2) if ups else (H, W)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, res, dy = rnd(2 * Bh, Hs, Ws, Cin, seed=1, dev=dev), rnd(2 * Bh, Ho, Wo, Cout, seed=2, dev=dev), rnd(2 * Bh, Ho, Wo, Cout, seed=3, dev=dev)
    rv = rnd(2 * Bh, Cout, seed=4, dev=dev).float()

    def run(rows, st, grouped):
        xg, rg, vg = x[rows].clone().requires_grad_(), res[rows].clone().requires_grad_(), rv[rows].clone().requires_grad_()
        with dual(pmap, grouped):
            y = ops.conv3x3_op(xg, st['weight'], st['bias'], st['w16'], st['w16t'], res=rg, rowvec=vg, stride=stride, ups=ups)
        y.backward(dy[rows])
        return y.detach(), xg.grad, rg.grad, vg.grad
    run.sets = (a, b)
    print(f'conv 2x{Bh} {H}x{W} {Cin}->{Cout} s{stride} u{ups}: y / dx / drowvec {_route(run, Bh, dy)}')


def _norm_conv(dev, Bh=1, H=8, W=12, C=160, N=160):
    from sid_lsg_amd import ops
    a, b, pmap = two_sets(dev, C, N, conv=True, e4m3=True)
    x, dy = rnd(2 * Bh, H, W, C, seed=1, dev=dev) * 2 + 0.5, rnd(2 * Bh, H, W, N, seed=2, dev=dev)
    rv = rnd(2 * Bh, N, seed=4, dev=dev).float()

    def run(rows, st, grouped, backward=True):
        xg, vg = x[rows].clone().requires_grad_(), rv[rows].clone().requires_grad_()
        with dual(pmap, grouped):
            y = ops.norm_conv_mx8(xg, st['gamma'], st['beta'], 1e-5, 8, st['w16'], st['bias'], st['w16t'], st['weight'], rowvec=vg)
        if backward:
            y.backward(dy[rows])
        return xg, vg, y
    return a, b, run


def test_norm_conv_mx8_single_form_returns_the_rowvec_gradient(dev):
    """1 x 8 x 12, 160 -> 160 channels, 8 groups, the row vector requires grad.  Before the single and the grouped e4m3 conv nodes
    were one node the single form returned None for the row vector (its grouped twin returned the gradient), so this test fails on
    that version: the gradient in both forms is the one intended change of behaviour of the fold."""
    a, b, run = _norm_conv(dev)
    _, vg, _ = run(slice(0, 2), a, True)
    for rows, st in ((slice(0, 1), a), (slice(1, 2), b)):
        _, v, _ = run(rows, st, False)
        assert v.grad is not None, 'the single form must return the row-vector gradient when it is asked for'
        print(f'drowvec sample {rows.start}: {same_or_close(v.grad, vg.grad[rows], "drowvec")}')


# ---------------------------------------------------------------------------------------------------------------- retention
def _check_saved(node, x, stats_shape, sets):
    """Grouped form: nothing but x and the statistics (stats_shape None: nothing at all) is saved -- no weight, no parameter."""
    saved = [t for t in node.saved_tensors if t is not None]
    forbidden = weight_shapes(sets[0]) | weight_shapes(sets[1])
    assert not [tuple(t.shape) for t in saved if tuple(t.shape) in forbidden], 'a weight is kept alive'
    got = sorted((t.data_ptr() == x.data_ptr(), tuple(t.shape), t.dtype) for t in saved)
    want = [] if stats_shape is None else sorted([(True, tuple(x.shape), x.dtype), (False, tuple(stats_shape), F32)])
    assert got == want, f'saved tensors {got}, expected {want}'


@pytest.mark.parametrize('op', ['linear', 'conv3x3_op', 'group_norm', 'layer_norm', 'norm_linear_mx8', 'norm_conv_mx8'])
def test_grouped_form_keeps_only_what_its_backward_reads(dev, op):
    """Phase B of the step runs the grouped pass on a stacked batch: an activation or a weight saved there for a weight gradient
    nobody computes is a memory regression.  linear / conv3x3_op: nothing; the norms and the e4m3 nodes: x and the statistics."""
    from sid_lsg_amd import ops
    if op == 'norm_conv_mx8':
        a, b, run = _norm_conv(dev)
        xg, _, y = run(slice(0, 2), a, True, backward=False)
        return _check_saved(y.grad_fn, xg, (2, 8, 2), (a, b))
    conv, e4m3 = op == 'conv3x3_op', op == 'norm_linear_mx8'
    C, N = (320, 320) if op in ('layer_norm', 'norm_linear_mx8') else (64, 160) if op in ('linear', 'conv3x3_op') else (160, 160)
    a, b, pmap = two_sets(dev, C, N, conv=conv, e4m3=e4m3)
    shape = {'linear': (128, 64), 'conv3x3_op': (2, 8, 8, 64), 'group_norm': (2, 8, 12, 160)}.get(op, (2, 64, 320))
    x = rnd(*shape, seed=1, dev=dev).requires_grad_()
    with ops.dual_networks(pmap):
        if op == 'linear':
            y, stats = ops.linear(x, a['weight'], a['bias'], a['w16'], a['w16t']), None
        elif op == 'conv3x3_op':
            y, stats = ops.conv3x3_op(x, a['weight'], a['bias'], a['w16'], a['w16t']), None
        elif op == 'group_norm':
            y, stats = ops.group_norm(x, a['gamma'], a['beta'], 8, 1e-5, True), (2, 8, 2)
        elif op == 'layer_norm':
            y, stats = ops.layer_norm(x, a['gamma'], a['beta']), (128, 2)
        else:
            y, stats = ops.norm_linear_mx8(x, a['gamma'], a['beta'], 1e-5, a['w16'], a['bias'], a['w16t'], a['weight']), (128, 2)
    _check_saved(y.grad_fn, x, stats, (a, b))


# ----------------------------------------------------------------------------------------------------------------- fallback
@pytest.mark.parametrize('rows_h', [77, 64])
@pytest.mark.parametrize('op', ['layer_norm', 'norm_linear_mx8'])
def test_grouped_layernorm_half_split_is_bit_equal(dev, op, rows_h):
    """C = 320; 77 rows per half: no multiple of 16, the halves run as two ordinary launches on the half views; 64: the two-set
    kernel.  LayerNorm is row-wise, so forward and input gradient equal the two single calls to the bit in both directions
    (test_gpu_grouped.py::test_grouped_layernorm_equals_two_launches asserts the same of the bf16 node at other sizes)."""
    from sid_lsg_amd import ops
    C = 320
    a, b, pmap = two_sets(dev, C, C, e4m3=op == 'norm_linear_mx8')
    x, dy = rnd(2 * rows_h, C, seed=1, dev=dev) * 2 + 0.5, rnd(2 * rows_h, C, seed=2, dev=dev)

    def run(rows, st, grouped):
        xg = x[rows].clone().requires_grad_()
        with dual(pmap, grouped):
            if op == 'layer_norm':
                y = ops.layer_norm(xg, st['gamma'], st['beta'])
            else:
                y = ops.norm_linear_mx8(xg, st['gamma'], st['beta'], 1e-5, st['w16'], st['bias'], st['w16t'], st['weight'])
        y.backward(dy[rows])
        return y.detach(), xg.grad
    y, dx = run(slice(0, 2 * rows_h), a, True)
    parts = [run(slice(0, rows_h), a, False), run(slice(rows_h, 2 * rows_h), b, False)]
    for got, ref, what in ((y, torch.cat([p[0] for p in parts]), 'forward'), (dx, torch.cat([p[1] for p in parts]), 'input gradient')):
        err = float((got.float() - ref.float()).abs().max())
        print(f'{op} 2x{rows_h} rows: {what} max difference {err:.3g}')
        assert torch.equal(got, ref), f'{op}, {rows_h} rows per half: {what} differs from the two single calls (max {err:.3g})'
    assert not torch.equal(y[rows_h:], run(slice(rows_h, 2 * rows_h), a, False)[0]), 'the second half must have used the second set'
