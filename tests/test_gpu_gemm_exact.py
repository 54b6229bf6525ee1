"""The bf16 GEMM / conv3x3 / weight-gradient kernels of csrc/gemm.hip, csrc/wgrad.hip and csrc/gemm_p8.h and the e4m3 GEMM / conv3x3 kernels of
csrc/gemm_fp8.hip on the EXACT cases of tests/gemm_cases.py: for
every table row the dispatch record must name the row's kernel, the result must equal the fp64 reference bit for bit (rounded once to
bf16, to nearest even, where the output is bf16), the sentinel around the output must be intact and no NaN of the poisoned padding,
guard rows or workspace may have reached the output.  Then the data-gradient chains of ops._conv_dgrad and one autograd pass each of
ops.linear and ops.conv3x3_op on exact data."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc      # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ids = lambda cases: [c['id'] for c in cases]      # noqa: E731


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


@pytest.fixture()
def ws(dev):
    """The split-K / pixel-split workspace at the size the table's records assume, NaN-filled by ws.poison()."""
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    buf = ops.ensure_workspace(dev)
    assert buf.numel() * 4 == gc.WORKSPACE_BYTES

    class Ws:
        def poison(self):
            buf.fill_(float('nan'))

        def shrink(self, nbytes):
            lib.sidlsg_set_workspace(buf.data_ptr(), nbytes)
    yield Ws()
    lib.sidlsg_set_workspace(buf.data_ptr(), buf.numel() * 4)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _forward_row(dev, ws, c):
    """Every call of a forward row (bf16 or e4m3): record, guard zones, no NaN, bit-equality."""
    from sid_lsg_amd._lib import lib
    M, N, K = gc.mnk(c)
    o, _ = gc.fwd_reference(c, 'plain')
    a2d = o['a'].reshape(-1, o['a'].shape[-1])
    a_pad, res_pad, rv_pad = {}, {}, {}
    _, w = gc.poisoned_flat(o['w'], dev)
    _, bias = gc.poisoned_flat(o['bias'], dev)
    w1 = bias1 = None
    if c['g2']:
        _, w1 = gc.poisoned_flat(o['w1'], dev)
        _, bias1 = gc.poisoned_flat(o['bias1'], dev)
    scales = {}
    if c['fp8']:                 # the scale vectors, NaN behind their last channel
        scale_bufs = {k: gc.poisoned_flat(o[k], dev)[1] for k in ('wscale', 'wscale1') if k in o}
        scales = {k: v.data_ptr() for k, v in scale_bufs.items()}
    errors = []
    old = lib.sidlsg_debug_set_p8.raw(c['p8'])
    try:
        for feat, rpb in gc.fwd_runs(c):
            f = gc.FEATS[feat]
            L = gc.fwd_layout(c, feat)
            pad = f['pad']
            if pad not in a_pad:
                a_pad[pad] = gc.poisoned(a2d, gc.a_pad_of(c, pad), dev)
            a = a_pad[pad]
            res = rv = None
            if f.get('res'):
                if pad not in res_pad:
                    res_pad[pad] = gc.poisoned(o['res'], gc.other_pad(pad), dev)
                res = res_pad[pad]
            if f.get('rv'):
                if (pad, rpb) not in rv_pad:
                    rv_pad[(pad, rpb)] = gc.poisoned(o['rv'][rpb], pad, dev)
                rv = rv_pad[(pad, rpb)]
            dtype = F32 if f.get('f32') else BF16
            whole, out = gc.guarded(M, N, pad, dtype, dev, fill=o['cprev'] if f.get('accum') else None)
            assert a.stride(0) == L['lda'] and out.stride(0) == L['ldc'] and (res is None or res.stride(0) == L['ldres']) and (rv is None or rv.stride(0) == L['ldrv'])
            p = dict(a=a.data_ptr(), w=w.data_ptr(), w1=w1.data_ptr() if c['g2'] else None, c=out.data_ptr(), bias=bias.data_ptr(),
                     bias1=bias1.data_ptr() if c['g2'] else None, res=None if res is None else res.data_ptr(), rv=None if rv is None else rv.data_ptr(), stream=_stream(),
                     **scales)
            name, args = gc.fwd_call(c, feat, rpb, p)
            ws.poison()
            if c['small_ws']:
                ws.shrink(gc.MX8_SMALL_WS_BYTES)
            try:
                getattr(lib, name)(*args)
            finally:
                if c['small_ws']:
                    ws.shrink(gc.WORKSPACE_BYTES)
            got_rec = gc.last_launch(lib)
            torch.cuda.synchronize()
            label = f"{c['id']} [{feat}/{rpb}]"
            _, x = gc.fwd_reference(c, feat, rpb)
            msgs = [gc.record_mismatch(label, got_rec, c['expect']), gc.guard_damage(whole, M, N)]
            got = out.contiguous()
            if f.get('silu'):
                msgs.append(gc.silu_mismatch(got.cpu(), x))
            else:
                msgs.append(gc.exact_mismatch(got, gc.round_out(x, dtype).to(dev)))
            errors += [f'{label}: {m}' for m in msgs if m]
    finally:
        lib.sidlsg_debug_set_p8.raw(old)
    assert not errors, '\n'.join(errors)


@pytest.mark.parametrize('c', gc.GEMM_CASES + gc.CONV_CASES, ids=ids(gc.GEMM_CASES + gc.CONV_CASES))
def test_forward_row(dev, ws, c):
    _forward_row(dev, ws, c)


@pytest.mark.parametrize('c', gc.FP8_CASES, ids=ids(gc.FP8_CASES))
def test_fp8_forward_row(dev, ws, c):
    """The e4m3 rows: operands as bytes, 0x7F (e4m3 NaN) in every padding byte and guard row of an e4m3 operand."""
    _forward_row(dev, ws, c)


def _wgrad_buffers(o, assign, dev):
    dy = gc.poisoned(o['dy'], gc.WG_PAD_Y, dev)
    a = gc.poisoned(o['a'].reshape(-1, o['a'].shape[-1]), gc.WG_PAD_A, dev)
    dw_prev = torch.full_like(o['dw_prev'], float('nan')) if assign else o['dw_prev']      # an assigning call must not read dW
    dw_whole, dw = gc.poisoned_flat(dw_prev, dev)
    db_whole, db = gc.poisoned_flat(o['db_prev'], dev)
    return dy, a, dw_whole, dw, db_whole, db


def _wgrad_judge(label, o, ref, assign, dw_whole, dw, db_whole, db, dev):
    dw_ref, db_ref = ref
    want_dw = gc.round_out(dw_ref + (0 if assign else o['dw_prev'].to(F64)), F32)
    want_db = gc.round_out(db_ref + o['db_prev'].to(F64), F32)
    msgs = [gc.exact_mismatch(dw, want_dw.to(dev)), gc.exact_mismatch(db, want_db.to(dev)), gc.flat_damage(dw_whole, dw.numel()), gc.flat_damage(db_whole, db.numel())]
    return [f'{label}: {m}' for m in msgs if m]


@pytest.mark.parametrize('c', gc.WGRAD_CASES, ids=ids(gc.WGRAD_CASES))
def test_wgrad_row(dev, ws, c):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    o = gc.wgrad_operands(c)
    ref = gc.wgrad_reference(c, o)
    errors = []
    with ops.deterministic(True if c['det'] else False):
        for assign in (0, 1):
            dy, a, dw_whole, dw, db_whole, db = _wgrad_buffers(o, assign, dev)
            name, args = gc.wgrad_call(c, assign, dict(dy=dy.data_ptr(), a=a.data_ptr(), dw=dw.data_ptr(), db=db.data_ptr(), stream=_stream()))
            ws.poison()
            if c['small_ws']:
                ws.shrink(gc.SMALL_WS_BYTES)
            try:
                getattr(lib, name)(*args)
            finally:
                ws.shrink(gc.WORKSPACE_BYTES)
            got_rec = gc.last_launch(lib)
            torch.cuda.synchronize()
            label = f"{c['id']} [assign={assign}]"
            m = gc.record_mismatch(label, got_rec, c['expect'])
            errors += ([m] if m else []) + _wgrad_judge(label, o, ref, assign, dw_whole, dw, db_whole, db, dev)
    assert not errors, '\n'.join(errors)


@pytest.mark.parametrize('c', gc.WGRAD_GROUPS, ids=ids(gc.WGRAD_GROUPS))
def test_wgrad_group(dev, ws, c):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    ops_ = gc.group_operands(c)
    bufs = [_wgrad_buffers(o, assign, dev) for o, (_, _, _, assign) in zip(ops_, c['jobs'])]
    jobs = gc.group_jobs(c, [(b[0].data_ptr(), b[1].data_ptr(), b[3].data_ptr(), b[5].data_ptr()) for b in bufs])
    ws.poison()
    with ops.deterministic(False):
        (lib.sidlsg_wgrad_group160_bf16 if c['t160'] else lib.sidlsg_wgrad_group_bf16)(ctypes.addressof(jobs), len(c['jobs']), _stream())
    got_rec = gc.last_launch(lib)
    torch.cuda.synchronize()
    errors = [m for m in [gc.record_mismatch(c['id'], got_rec, c['expect'])] if m]
    for i, (o, (M, N, K, assign), b) in enumerate(zip(ops_, c['jobs'], bufs)):
        ref = gc.wgrad_reference(dict(ep='wgrad'), o)
        errors += _wgrad_judge(f"{c['id']} job {i} ({M}x{N}x{K})", o, ref, assign, b[2], b[3], b[4], b[5], dev)
    assert not errors, '\n'.join(errors)


# (B, Hs, Ws, Cin, Cout, stride, ups): odd sizes under stride 2 (the zero-inserted image is one row / column short of 2 Ho x 2 Wo), an upsampled conv
DGRAD = [(3, 9, 7, 72, 40, 2, 0), (2, 12, 20, 64, 160, 2, 0), (2, 6, 10, 64, 160, 1, 1), (2, 12, 20, 8, 320, 1, 0)]


@pytest.mark.parametrize('B,Hs,Ws,Cin,Cout,stride,ups', DGRAD)
def test_conv_dgrad_chain(dev, ws, B, Hs, Ws, Cin, Cout, stride, ups):
    from sid_lsg_amd import ops
    g = torch.Generator().manual_seed(11 + B * Hs + Cin)
    H, W = (2 * Hs, 2 * Ws) if ups else (Hs, Ws)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    w = gc.ints(g, (Cout, 9 * Cin), -2, 2, BF16)
    dy = gc.ints(g, (B, Ho, Wo, Cout), -3, 3, BF16)
    want = gc.dgrad_reference(dy, w, (B, Hs, Ws, Cin), stride, ups)
    w16t = ops.transpose_w(w.float().to(dev), Cout, Cin, 9)
    assert torch.equal(w16t.cpu().view(Cin, 9 * Cout), gc.transpose_taps(w, Cout, Cin)), 'sidlsg_transpose_w'
    ws.poison()
    dx = ops._conv_dgrad(dy.to(dev), w16t.view(Cin, 9 * Cout), (B, Hs, Ws, Cin), stride, ups, BF16)
    torch.cuda.synchronize()
    msg = gc.exact_mismatch(dx, want.to(dev))
    assert not msg, msg


def test_linear_autograd_exact(dev, ws):
    from sid_lsg_amd import ops
    M, N, K = 1030, 136, 72
    g = torch.Generator().manual_seed(3)
    x, w, dy = gc.ints(g, (M, K), -3, 3, BF16), gc.ints(g, (N, K), -2, 2, BF16), gc.ints(g, (M, N), -3, 3, BF16)
    bias, res = gc.ints(g, (N,), -1000, 1000, F32), gc.ints(g, (M, N), -1000, 1000, BF16)
    wm = torch.nn.Parameter(w.float().to(dev)); wm.grad = torch.zeros_like(wm)
    bm = torch.nn.Parameter(bias.to(dev)); bm.grad = torch.zeros_like(bm)
    xd, rd = x.to(dev).requires_grad_(), res.to(dev).requires_grad_()
    ws.poison()
    y = ops.linear(xd, wm, bm, w.to(dev), ops.transpose_w(wm, N, K, 1), res=rd)
    y.backward(dy.to(dev))
    ops.flush_wgrad_queues()
    torch.cuda.synchronize()
    x64, w64, dy64 = x.to(F64), w.to(F64), dy.to(F64)
    want = dict(y=(gc.round_out(x64 @ w64.t() + bias.to(F64) + res.to(F64), BF16), y), dx=(gc.round_out(dy64 @ w64, BF16), xd.grad), dres=(dy, rd.grad),
                dW=(gc.round_out(dy64.t() @ x64, F32), wm.grad), db=(gc.round_out(dy64.sum(0), F32), bm.grad))
    errors = [f'{k}: {m}' for k, (ref, got) in want.items() for m in [gc.exact_mismatch(got.detach(), ref.to(dev))] if m]
    assert not errors, '\n'.join(errors)


@pytest.mark.parametrize('stride,ups', [(1, 0), (2, 0), (1, 1)])
def test_conv_autograd_exact(dev, ws, stride, ups):
    from sid_lsg_amd import ops
    B, Hs, Ws, Cin, Cout = 3, 10, 6, 72, 136
    c = dict(ep='conv', B=B, Hs=Hs, Ws=Ws, Cin=Cin, Cout=Cout, stride=stride, ups=ups)
    H, W, Ho, Wo = gc.conv_geometry(c)
    g = torch.Generator().manual_seed(7 + stride + ups)
    x, w, dy = gc.ints(g, (B, Hs, Ws, Cin), -3, 3, BF16), gc.ints(g, (Cout, 9 * Cin), -2, 2, BF16), gc.ints(g, (B, Ho, Wo, Cout), -3, 3, BF16)
    bias, rv = gc.ints(g, (Cout,), -1000, 1000, F32), gc.ints(g, (B, Cout), -300, 300, F32)
    wm = torch.nn.Parameter(w.float().view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).to(dev))          # logical [Cout, Cin, 3, 3], channels-last storage
    wm.grad = torch.zeros(Cout, 3, 3, Cin, device=dev).permute(0, 3, 1, 2)
    bm = torch.nn.Parameter(bias.to(dev)); bm.grad = torch.zeros_like(bm)
    xd, rvd = x.to(dev).requires_grad_(), rv.to(dev).requires_grad_()
    ws.poison()
    y = ops.conv3x3_op(xd, wm, bm, w.to(dev), ops.transpose_w(wm.permute(0, 2, 3, 1), Cout, Cin, 9), None, rvd, stride, ups, False)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    acc = gc.contract(c, x, w) + bias.to(F64) + rv.to(F64).repeat_interleave(Ho * Wo, 0)
    dw, db = gc.wgrad_reference(c, dict(a=x, dy=dy.view(-1, Cout)))
    want = dict(y=(gc.round_out(acc, BF16).view(B, Ho, Wo, Cout), y), dx=(gc.dgrad_reference(dy, w, (B, Hs, Ws, Cin), stride, ups), xd.grad),
                dW=(gc.round_out(dw, F32), wm.grad.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)), db=(gc.round_out(db, F32), bm.grad),
                drv=(gc.round_out(dy.to(F64).sum(dim=(1, 2)), F32), rvd.grad))
    errors = [f'{k}: {m}' for k, (ref, got) in want.items() for m in [gc.exact_mismatch(got.detach().contiguous(), ref.to(dev))] if m]
    assert not errors, '\n'.join(errors)
