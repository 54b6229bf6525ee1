"""The fused d = 40 attention backward (csrc/attention.hip: attn_delta_kernel + attn_bwd_fused_kernel + attn_dq_reduce_kernel), forced on
with sidlsg_debug_set_attn_bwd_fused(2) (every shape the kernel can run, no length threshold) and checked, plain and `_ps`, against
  (a) the fp32 reference attn_ref of tests/test_gpu_ops.py with that file's close(..., 2e-2),
  (b) the two-kernel path on the same inputs: the fused gradients may lie no further from the fp32 reference than the two-kernel
      ones plus 10 % (distance = l2 norm of the difference over the whole tensor: the two paths add dQ in a different order and
      delta in a different order, so single elements round differently and a maximum over elements would compare two draws of
      rounding noise; the norm averages over >= 20 000 elements),
  (c) itself: two runs are bit-identical (the slabs are added in index order).
Shapes: the smallest that reach each hazard -- one 512-key group (reduce over one slab); two groups x several heads and batches (slab
indexing, strides); three groups with q|k|v packed in one [B, N, 3C] buffer as ops.self_attention passes it (ld != C).  Calls the
rule refuses must give the bits of the switched-off path."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
LOG2E = 1.4426950408889634
SHAPES = [(1, 1, 512, 40, False), (2, 3, 1024, 40, False), (1, 2, 1536, 40, True)]      # B, heads, N, D, packed


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    lib.load()
    d = torch.device('cuda:0')
    ops.ensure_workspace(d)          # the slabs live in the split-K workspace
    return d


@pytest.fixture()
def fused(dev):
    """fused.set(mode): 0 two kernels, 2 fused wherever the kernel can run; the setting is restored afterwards."""
    from sid_lsg_amd._lib import lib

    class Ctl:
        def set(self, mode):
            lib.sidlsg_debug_set_attn_bwd_fused.raw(mode)

        def takes(self, B, H, Nq, Nk, D, kv=True):
            return lib.sidlsg_attn_bwd_fused_takes.raw(B, H, Nq, Nk, D, 1 if kv else 0) == 1
    old = lib.sidlsg_debug_set_attn_bwd_fused.raw(-1)
    yield Ctl()
    lib.sidlsg_debug_set_attn_bwd_fused.raw(old)


def make_inputs(B, heads, N, D, packed, ps, seed=1, special=False):
    """-> (q, k, v, do) bf16 on the CPU (views of one [B, N, 3C] buffer when packed) and the fp32 tensors the kernel's arithmetic sees."""
    from test_gpu_ops import rnd
    C = heads * D
    qkv = rnd(B, N, 3 * C, seed=seed)
    if special:              # the input of test_self_attention_prescaled_queries: one key far above the rest, in the middle
        qkv[:, N // 2 + 3, C:C + D] *= 12.0
        qkv[:, :, 0] -= 0.5
    c = D ** -0.5 * LOG2E
    if ps:
        qkv[..., :C] = (qkv[..., :C].float() * c).to(BF16)
    do = rnd(B, N, C, seed=seed + 1)
    return qkv, do, c


def reference(qkv, do, heads, ps, c):
    from test_gpu_ops import attn_ref
    C = qkv.shape[2] // 3
    r = qkv.float()
    if ps:
        r[..., :C] /= c          # the unscaled queries
    r.requires_grad_()
    attn_ref(r[..., :C], r[..., C:2 * C], r[..., 2 * C:], heads).backward(do.float())
    return r.grad[..., :C], r.grad[..., C:2 * C], r.grad[..., 2 * C:]


def run_bwd(dev, qkv, do, heads, ps, packed, kv=True):
    """forward + backward through the C entry points -> (dq, dk, dv) on the CPU.  packed: q, k, v are column slices of the one
    buffer (token stride 3C); else three contiguous tensors (token stride C)."""
    from sid_lsg_amd._lib import lib
    B, N, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    sfx = '_ps' if ps else ''
    s = torch.cuda.current_stream().cuda_stream
    if packed:
        buf = qkv.to(dev)
        g = torch.zeros_like(buf)
        ptr = [buf.data_ptr() + 2 * C * i for i in range(3)]
        gptr = [g.data_ptr() + 2 * C * i for i in range(3)]
        ld = C3
    else:
        parts = [qkv[..., i * C:(i + 1) * C].contiguous().to(dev) for i in range(3)]
        grads = [torch.zeros_like(t) for t in parts]
        ptr = [t.data_ptr() for t in parts]
        gptr = [t.data_ptr() for t in grads]
        ld = C
    dod = do.to(dev)
    o = torch.empty(B, N, C, device=dev, dtype=BF16)
    lse = torch.empty(B, heads, N, device=dev, dtype=F32)
    delta = torch.empty(B, heads, N, device=dev, dtype=F32)
    getattr(lib, 'sidlsg_attn_fwd' + sfx)(ptr[0], ptr[1], ptr[2], o.data_ptr(), lse.data_ptr(), B, heads, N, N, D, ld, ld, ld, C,
                                          N * ld, N * ld, N * ld, N * C, s)
    getattr(lib, 'sidlsg_attn_bwd' + sfx)(ptr[0], ptr[1], ptr[2], o.data_ptr(), dod.data_ptr(), lse.data_ptr(), gptr[0],
                                          gptr[1] if kv else None, gptr[2] if kv else None, delta.data_ptr(), B, heads, N, N, D,
                                          ld, ld, ld, C, N * ld, N * ld, N * ld, N * C, s)
    torch.cuda.synchronize()
    if packed:
        gc = g.cpu()
        return gc[..., :C], gc[..., C:2 * C], gc[..., 2 * C:]
    return tuple(t.cpu() for t in grads)


_cache = {}


def case(dev, fused, shape, ps):
    """reference, two-kernel and fused gradients of a shape: computed once, shared by the tests, never modified"""
    key = (shape, ps)
    if key not in _cache:
        B, heads, N, D, packed = shape
        qkv, do, c = make_inputs(B, heads, N, D, packed, ps)
        ref = reference(qkv, do, heads, ps, c)
        fused.set(0)
        assert not fused.takes(B, heads, N, N, D)
        two = run_bwd(dev, qkv, do, heads, ps, packed)
        fused.set(2)
        assert fused.takes(B, heads, N, N, D), 'the fused path did not take this shape'
        one = run_bwd(dev, qkv, do, heads, ps, packed)
        again = run_bwd(dev, qkv, do, heads, ps, packed)
        _cache[key] = (ref, two, one, again)
    return _cache[key]


@pytest.mark.parametrize('ps', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_fused_backward_matches_fp32_reference(dev, fused, shape, ps):
    from test_gpu_ops import close
    ref, _, one, _ = case(dev, fused, shape, ps)
    for name, g, r in zip(('dq', 'dk', 'dv'), one, ref):
        close(g, r, 2e-2, name)


@pytest.mark.parametrize('ps', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_fused_backward_is_as_close_as_two_kernels(dev, fused, shape, ps):
    ref, two, one, _ = case(dev, fused, shape, ps)
    for name, g1, g2, r in zip(('dq', 'dk', 'dv'), one, two, ref):
        e1, e2 = (g1.float() - r).norm().item(), (g2.float() - r).norm().item()
        print(f'{shape} ps={ps} {name}: |fused - ref| {e1:.6g}  |two-kernel - ref| {e2:.6g}  ratio {e1 / e2:.4f}')
        assert e1 <= 1.10 * e2, f'{name}: fused {e1:.6g} vs two-kernel {e2:.6g} from the fp32 reference'


@pytest.mark.parametrize('ps', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_fused_backward_is_bit_reproducible(dev, fused, shape, ps):
    _, _, one, again = case(dev, fused, shape, ps)
    for name, a, b in zip(('dq', 'dk', 'dv'), one, again):
        assert torch.equal(a, b), name


@pytest.mark.parametrize('shape', SHAPES[:2])
def test_fused_backward_running_maximum_jump(dev, fused, shape):
    """The `_ps` input of test_self_attention_prescaled_queries: the row maximum jumps by > 2^8 between key tiles."""
    from test_gpu_ops import close
    B, heads, N, D, packed = shape
    qkv, do, c = make_inputs(B, heads, N, D, packed, True, special=True)
    ref = reference(qkv, do, heads, True, c)
    fused.set(2)
    assert fused.takes(B, heads, N, N, D)
    for name, g, r in zip(('dq', 'dk', 'dv'), run_bwd(dev, qkv, do, heads, True, packed), ref):
        close(g, r, 2e-2, name)


@pytest.mark.parametrize('ps', [False, True])
def test_fused_backward_all_negative_score_row(dev, fused, ps):
    from test_gpu_ops import close
    B, heads, N, D = 1, 1, 512, 40
    qkv, do, c = make_inputs(B, heads, N, D, False, False, seed=5)
    qkv[:, :, D] = 2.0                       # k[:, 0] = 2 for every key
    qkv[:, 7, :D] = 0.0
    qkv[:, 7, 0] = -30.0                     # query 7: every score = -60 / sqrt(40)
    if ps:
        qkv[..., :D] = (qkv[..., :D].float() * c).to(BF16)
    ref = reference(qkv, do, heads, ps, c)
    fused.set(2)
    assert fused.takes(B, heads, N, N, D)
    for name, g, r in zip(('dq', 'dk', 'dv'), run_bwd(dev, qkv, do, heads, ps, False), ref):
        close(g, r, 2e-2, name)


def test_fused_backward_propagates_nan(dev, fused):
    """As test_attention_propagates_nan: a NaN in one q row of sample 1 surfaces in that sample's gradients and leaves sample 0's bits alone."""
    B, heads, N, D = 2, 1, 512, 40
    qkv, do, _ = make_inputs(B, heads, N, D, False, False, seed=7)
    fused.set(2)
    assert fused.takes(B, heads, N, N, D)
    clean = run_bwd(dev, qkv, do, heads, False, False)
    bad = qkv.clone()
    bad[1, 17, 3] = float('nan')
    got = run_bwd(dev, bad, do, heads, False, False)
    for name, g, cl in zip(('dq', 'dk', 'dv'), got, clean):
        assert torch.isnan(g[1]).any(), name
        assert torch.equal(g[0], cl[0]), name


@pytest.mark.parametrize('B,heads,N,D,kv', [(2, 2, 200, 40, True), (1, 2, 512, 80, True), (1, 2, 512, 40, False)])
def test_refused_calls_keep_the_two_kernel_path(dev, fused, B, heads, N, D, kv):
    """Ragged N, d = 80 and a dQ-only call: the rule refuses them and the result is the switched-off path's, bit for bit."""
    qkv, do, _ = make_inputs(B, heads, N, D, True, False, seed=9)
    fused.set(0)
    off = run_bwd(dev, qkv, do, heads, False, True, kv=kv)
    fused.set(2)
    assert not fused.takes(B, heads, N, N, D, kv)
    on = run_bwd(dev, qkv, do, heads, False, True, kv=kv)
    for a, b in zip(off, on):
        assert torch.equal(a, b)


def test_rule_mode_and_batch_chunks(dev, fused):
    """Mode 1 (by rule) keeps short sequences on the two-kernel path; a workspace too small for the whole batch's slabs is walked in
    chunks with the same bits."""
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    fused.set(1)
    assert not fused.takes(2, 3, 1024, 1024, 40) and fused.takes(8, 8, 4096, 4096, 40)
    shape = SHAPES[1]
    B, heads, N, D, packed = shape
    _, _, one, _ = case(dev, fused, shape, False)
    qkv, do, _ = make_inputs(B, heads, N, D, packed, False)
    ws = ops.ensure_workspace(dev)
    per_b = heads * (N // 512) * N * D * 4
    try:
        lib.sidlsg_set_workspace(ws.data_ptr(), per_b + 1024)      # room for one batch element only
        fused.set(2)
        assert fused.takes(B, heads, N, N, D)
        got = run_bwd(dev, qkv, do, heads, False, packed)
    finally:
        lib.sidlsg_set_workspace(ws.data_ptr(), ws.numel() * 4)
    for a, b in zip(one, got):
        assert torch.equal(a, b)
