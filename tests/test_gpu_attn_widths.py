"""Attention at every admitted head width, with keys that can be told apart (tests/attn_cases.py has the inputs, the fp64 reference,
the bounds and how they were derived; tests/test_attn_cases_host.py proves on the CPU that these tests can fail).

  * head-width sweep: ops.self_attention on the packed [B, N, 3C] buffer, plain and `_ps`, forward and all three gradients, for
    every D the dispatcher admits (16 widths: both members of every DP pair, so the ones-column forward and the plain forward of
    every DP), N = 200 and N = 128, needle inputs;
  * length edges at D = 8, 40, 48, 96, 128, 160: self-attention N = 1 .. 129, cross-attention with 1 .. 128 keys, 1032 keys at
    D = 40 / 48 (attn_dkdv_kernel<48, 2>), the dQ-only backward at D = 96 / 128;
  * masking: the forward with the LSE on the biased inputs (a phantom key would weigh e^12 real ones), every edge shape;
  * the fused backward at D = 48 (it had only run at D = 40);
  * the causal kernels (bf16 and fp32) at D = 8 .. 128 and the fp32 attention at ten widths;
  * the contract: widths without a kernel return -22 from all four entry points, write nothing, and ops says so in words.

Every comparison is per (batch, head) slice (attn_cases.close_slices) AND over the whole tensor (close() of tests/test_gpu_ops.py).
`pytest -s` prints every figure and, at the end, the largest ones."""
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
EINVAL = -22
_worst = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    lib.load()
    d = torch.device('cuda:0')
    ops.ensure_workspace(d)          # the fused backward's slabs live in the split-K workspace
    yield d
    print('\nlargest figures of this run: ' + '  '.join(f'{k}={v[0]:.5f} ({v[1]})' for k, v in sorted(_worst.items())))


@pytest.fixture()
def fused(dev):
    """As the fixture of tests/test_gpu_attn_bwd_fused.py: fused.set(2) takes every shape the kernel can run; restored afterwards."""
    from sid_lsg_amd._lib import lib

    class Ctl:
        def set(self, mode):
            lib.sidlsg_debug_set_attn_bwd_fused.raw(mode)

        def takes(self, B, H, Nq, Nk, D):
            return lib.sidlsg_attn_bwd_fused_takes.raw(B, H, Nq, Nk, D, 1)
    old = lib.sidlsg_debug_set_attn_bwd_fused.raw(-1)
    yield Ctl()
    lib.sidlsg_debug_set_attn_bwd_fused.raw(old)


def _note(key, val, what):
    if val > _worst.get(key, (-1.0, ''))[0]:
        _worst[key] = (val, what)


def run_ops(dev, c, x, need_kv=True):
    """Forward and backward through ops.self_attention / ops.cross_attention -> dict(o, dq, dk, dv) on the CPU (dk = dv = None when
    the keys / values take no gradient: the dQ-only backward)."""
    from sid_lsg_amd import ops
    C = c.H * c.D
    if c.kind == 'self':
        qd = x['qkv'].to(dev).requires_grad_()
        y = ops.self_attention(qd, c.H, prescaled=c.ps)
        y.backward(x['do'].to(dev))
        g = qd.grad.cpu()
        return dict(o=y.detach().cpu(), dq=g[..., :C], dk=g[..., C:2 * C], dv=g[..., 2 * C:])
    qd, kd = x['q'].to(dev).requires_grad_(), x['kv'].to(dev).requires_grad_(need_kv)
    y = ops.cross_attention(qd, kd, c.H, prescaled=c.ps)
    y.backward(x['do'].to(dev))
    out = dict(o=y.detach().cpu(), dq=qd.grad.cpu(), dk=None, dv=None)
    if need_kv:
        g = kd.grad.cpu()
        out.update(dk=g[..., :C], dv=g[..., C:])
    else:
        assert kd.grad is None
    return out


def check(c, got, ref, tol_o=ac.FWD_TOL, tol_g=ac.GRAD_TOL, tol_whole=ac.WHOLE_GRAD_TOL, tag=''):
    """Per slice at the derived bounds, then the whole tensor as tests/test_gpu_ops.py does (not where the reference is identically
    zero, dQ and dK over one key: close_slices has an absolute bound for that)."""
    from test_gpu_ops import close
    what = ac.case_id(c) + tag
    errs = {}
    for n in ('o', 'dq', 'dk', 'dv'):
        if got.get(n) is None:
            continue
        errs[n] = ac.slice_rel_err(got[n], ref[n], c.H)
        _note(('f32 ' if tol_o < 1e-3 else '') + n, errs[n], what)
    print(f'  {what}: ' + ' '.join(f'{n}={v:.5f}' for n, v in errs.items()))
    for n, e in errs.items():
        tol = tol_o if n == 'o' else tol_g[n]
        assert e <= tol, f'{what} {n}: per-(batch, head) max err / max|ref| = {e:.3g} > {tol}'
        if ref[n].abs().max().item() > 1e-12:
            close(got[n], ref[n], tol_o if n == 'o' else tol_whole, f'{what} {n} (whole tensor)')


# ---- head-width sweep and length edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', ac.SWEEP_CASES, ids=ac.case_id)
def test_width_sweep(dev, c):
    x, ref = ac.case_data(c)
    check(c, run_ops(dev, c, x), ref)


@pytest.mark.parametrize('c', ac.EDGE_CASES + ac.LONG_CASES, ids=ac.case_id)
def test_length_edges(dev, c):
    x, ref = ac.case_data(c)
    check(c, run_ops(dev, c, x), ref)


@pytest.mark.parametrize('c', ac.DQ_ONLY_CASES, ids=ac.case_id)
def test_query_gradient_only(dev, c):
    """Keys and values that take no gradient: ops passes dK = dV = NULL and only the dQ kernel runs."""
    x, ref = ac.case_data(c)
    got = run_ops(dev, c, x, need_kv=False)
    assert got['dk'] is None and got['dv'] is None
    check(c, got, ref, tag=' dq-only')


# ---- masking: forward and LSE on the biased inputs ---------------------------------------------------------------------------------
def raw_forward(dev, c, x):
    """sidlsg_attn_fwd(_ps) on the case's buffers in place (packed q | k | v: token stride 3C) -> (o, lse2) on the CPU."""
    from sid_lsg_amd._lib import lib
    C = c.H * c.D
    if c.kind == 'self':
        buf = x['qkv'].to(dev)
        q, k, v = buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:]
    else:
        q, kvb = x['q'].to(dev), x['kv'].to(dev)
        k, v = kvb[..., :C], kvb[..., C:]
    o = torch.full((c.B, c.Nq, C), float('nan'), device=dev, dtype=BF16)
    lse = torch.full((c.B, c.H, c.Nq), float('nan'), device=dev, dtype=F32)
    getattr(lib, 'sidlsg_attn_fwd' + ('_ps' if c.ps else ''))(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), c.B, c.H, c.Nq, c.Nk, c.D, q.stride(1), k.stride(1), v.stride(1), C,
        q.stride(0), k.stride(0), v.stride(0), c.Nq * C, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


@pytest.mark.parametrize('c', ac.BIASED_CASES, ids=ac.case_id)
def test_masking_forward_and_lse(dev, c):
    """Every score 12 nats below a zero row's: a key row read past Nk that escaped the mask would take the whole softmax.  The LSE
    comes back in the log2 domain (m + log2 l) and is compared with the fp64 log-sum-exp."""
    from test_gpu_ops import close
    x, ref = ac.case_data(c, kind='biased', grads=False)
    o, lse = raw_forward(dev, c, x)
    eo, el = ac.slice_rel_err(o, ref['o'], c.H), ac.lse_err_bits(lse, ref['lse2'])
    print(f'  {ac.case_id(c)} biased: o={eo:.5f} lse={el:.5f} bits')
    _note('biased o', eo, ac.case_id(c))
    _note('lse bits', el, ac.case_id(c))
    assert eo <= ac.FWD_TOL, f'o: per-(batch, head) max err / max|ref| = {eo:.3g} > {ac.FWD_TOL}'
    close(o, ref['o'], ac.FWD_TOL, 'o (whole tensor)')
    assert el <= ac.LSE_TOL_BITS, f'LSE off by {el:.3g} bits > {ac.LSE_TOL_BITS}'


# ---- fused backward at D = 48 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', ac.FUSED_CASES, ids=ac.case_id)
def test_fused_backward_d48(dev, fused, c):
    x, ref = ac.case_data(c)
    fused.set(2)
    assert fused.takes(c.B, c.H, c.Nq, c.Nk, c.D) == 1, 'the fused path did not take this shape'
    got = run_ops(dev, c, x)
    again = run_ops(dev, c, x)
    check(c, got, ref, tag=' fused')
    for n in ('dq', 'dk', 'dv'):
        assert torch.equal(got[n], again[n]), f'{n}: two runs differ'


# ---- causal kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('c', ac.CAUSAL_CASES, ids=ac.case_id)
def test_causal_widths(dev, c, dtype):
    """Needles at keys 0, 15, 16 and N - 1: the queries in front of a needle must not see it (they are rows of the same comparison)."""
    from sid_lsg_amd import ops
    x, ref = ac.case_data(c, dtype=dtype, causal=True, grads=False)
    got = ops.causal_self_attention(x['qkv'].to(dev), c.H).cpu()
    tol = ac.FWD_TOL if dtype == BF16 else ac.F32_TOL['o']
    e = ac.slice_rel_err(got, ref['o'], c.H)
    print(f'  causal {ac.case_id(c)} {dtype}: o={e:.3g}')
    _note('causal o' if dtype == BF16 else 'f32 causal o', e, ac.case_id(c))
    assert e <= tol, f'per-(batch, head) max err / max|ref| = {e:.3g} > {tol}'


# ---- fp32 attention ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', ac.F32_CASES, ids=ac.case_id)
def test_f32_widths(dev, c):
    x, ref = ac.case_data(c, dtype=F32)
    got = run_ops(dev, c, x)
    assert got['o'].dtype == F32
    check(c, got, ref, tol_o=ac.F32_TOL['o'], tol_g=ac.F32_TOL, tol_whole=ac.F32_TOL['dq'], tag=' f32')


# ---- contract: the widths without a kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('ps', [False, True], ids=['plain', 'ps'])
@pytest.mark.parametrize('D', ac.REFUSED_WIDTHS)
def test_refused_widths_return_einval_and_write_nothing(dev, D, ps):
    from sid_lsg_amd._lib import lib
    B, H, N = 1, 2, 32
    C = H * max(D, 8)
    sfx = '_ps' if ps else ''
    s = torch.cuda.current_stream().cuda_stream
    q, k, v, do = (torch.randn(B, N, C, device=dev).to(BF16) for _ in range(4))
    poison = lambda *shape, dt=BF16: torch.full(shape, float('nan'), device=dev, dtype=dt)      # noqa: E731
    o, dq, dk, dv = (poison(B, N, C) for _ in range(4))
    lse, delta = poison(B, H, N, dt=F32), poison(B, H, N, dt=F32)
    before = [t.clone() for t in (o, dq, dk, dv, lse, delta)]
    rc = getattr(lib, 'sidlsg_attn_fwd' + sfx).raw(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, N, N, D, C, C, C, C,
                                                  N * C, N * C, N * C, N * C, s)
    assert rc == EINVAL, f'forward, D = {D}: {rc}'
    lse_in = torch.zeros(B, H, N, device=dev, dtype=F32)
    o_in = torch.zeros(B, N, C, device=dev, dtype=BF16)
    for kv in (True, False):
        rc = getattr(lib, 'sidlsg_attn_bwd' + sfx).raw(q.data_ptr(), k.data_ptr(), v.data_ptr(), o_in.data_ptr(), do.data_ptr(), lse_in.data_ptr(),
                                                      dq.data_ptr(), dk.data_ptr() if kv else None, dv.data_ptr() if kv else None, delta.data_ptr(),
                                                      B, H, N, N, D, C, C, C, C, N * C, N * C, N * C, N * C, s)
        assert rc == EINVAL, f'backward, D = {D}, dK / dV {kv}: {rc}'
    torch.cuda.synchronize()
    for name, t, b in zip(('O', 'dQ', 'dK', 'dV', 'LSE', 'delta'), (o, dq, dk, dv, lse, delta), before):
        it = torch.int16 if t.dtype == BF16 else torch.int32
        assert torch.equal(t.view(it), b.view(it)), f'{name} was written'


def test_ops_names_the_admitted_widths(dev):
    from sid_lsg_amd import ops
    assert ops.ATTN_HEAD_WIDTHS == ac.ADMITTED_DP
    for D, dtype in ((104, BF16), (112, BF16), (136, BF16), (144, BF16), (4, BF16), (168, BF16), (104, F32), (6, F32), (164, F32)):
        qkv = torch.zeros(1, 16, 3 * 2 * D, device=dev, dtype=dtype)
        with pytest.raises(RuntimeError, match=r'head width \d+ is not admitted.*16, 32, 48, 64, 80, 96, 128, 160'):
            ops.self_attention(qkv, 2)
        with pytest.raises(RuntimeError, match='not admitted'):
            ops.cross_attention(qkv[..., :2 * D].contiguous(), qkv[..., :4 * D].contiguous(), 2)
    with pytest.raises(RuntimeError, match='not admitted'):
        ops.self_attention(torch.zeros(1, 16, 3 * 2 * 104, device=dev, dtype=BF16), 2, prescaled=True)
    # the header says the same: the sentence the message paraphrases
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sidlsg_hip.h')).read()
    assert 'round-up to a multiple of 16 is one of 16, 32, 48, 64, 80, 96, 128 or 160' in header
    for D in ac.WIDTHS:            # and every admitted width runs
        y = ops.self_attention(torch.zeros(1, 16, 3 * 2 * D, device=dev, dtype=BF16), 2)
        assert y.shape == (1, 16, 2 * D)
