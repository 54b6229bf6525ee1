"""Small chains of the project's ops with their fp32 CPU twins, shared by tests/test_gpu_backward_state.py and its worker process
(tests/backward_state_worker.py).  Not a test module.

Every leaf stage has `.gpu(x)` (the HIP op), `.ref(x)` (plain torch, fp32, CPU) and `.params()`.

The reference is the fp32 CPU twin of every op of the chain, run with torch autograd AT THE TENSORS THE HIP CHAIN STORED: taps around
each op record its bf16 input, its output and the gradient that reached it, and the twin is evaluated on exactly those (bf16 is exact
in fp32, the accumulation is fp32 on both sides).  That is the convention the suite's bounds come from (test_gpu_ops.py: 2e-3 of
max|ref| for fp32 parameter gradients, 1.2e-2 for bf16 tensors: one rounding), and it is the only way a chain can meet them: in a
free-running fp32 chain every bf16 store of the HIP chain is a 2^-9 relative perturbation, one-ulp differences multiply from layer to
layer, and the gradient that reaches the first of nine ops differs by ~5e-3 per element from the fp32 one -- more than the bound,
with nothing wrong.  Run this way, each parameter gradient is checked against the sum over ALL uses of the parameter in the pass
(the twin's leaves accumulate), so a contribution that is dropped, applied twice or left over from another pass is an error of the
order of the gradient itself -- which is why every comparison first asserts that the reference gradient is not zero.
"""
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

BF16, F32 = torch.bfloat16, torch.float32
DEV = 'cuda:0'
TOL_F32, TOL_BF16 = 2e-3, 1.2e-2


def close(got, ref, tol, name=''):
    """test_gpu_ops.close: max error against max|ref|."""
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-12
    print(f'  {name}: max err {err:.4g}, scale {scale:.4g}, rel {err / scale:.3g} (bound {tol})')
    assert err <= tol * scale, f'{name}: max err {err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g} > {tol})'


def randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class _Tap(torch.autograd.Function):
    """Identity that records what passes: the tensor on the way forward (entry[fwd]), the gradient on the way back (entry[bwd])."""

    @staticmethod
    def forward(ctx, x, entry, fwd, bwd):
        ctx.entry, ctx.bwd = entry, bwd
        entry[fwd] = x.detach()
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.entry[ctx.bwd] = g.detach()
        return g, None, None, None


_record = None          # the list the running HIP chain appends one entry per executed op to (Model.backward)


def tapped(stage, x, *more):
    """stage.gpu(x, *more) between two taps -> its output.  An op that is executed without a backward of its own (the no-grad
    forward of a checkpoint, a recomputation) leaves an entry without 'dy'."""
    entry = {'stage': stage, 'more': more}
    _record.append(entry)
    y = stage.gpu(_Tap.apply(x, entry, 'x', 'dx'), *more)
    return _Tap.apply(y, entry, 'y', 'dy')


def _param(t):
    p = torch.nn.Parameter(t.to(DEV))
    p.grad = torch.zeros_like(p)
    return p


class Lin:
    """K -> N Linear (fp32 master = its bf16 compute copy, exactly)."""
    leaf = True

    def __init__(self, name, n, k, seed):
        self.name = name
        w = (randn((n, k), seed) * k ** -0.5).to(BF16).float()
        b = randn((n,), seed + 1000, 0.1)
        self.rw, self.rb = w.clone().requires_grad_(), b.clone().requires_grad_()
        self.w, self.b = _param(w), _param(b)
        self.w16 = self.w.detach().to(BF16)
        self.w16t = self.w16.t().contiguous()

    def gpu(self, x):
        from sid_lsg_amd import ops
        return ops.linear(x, self.w, self.b, self.w16, self.w16t)

    def ref(self, x):
        return F.linear(x, self.rw, self.rb)

    def params(self):
        return [(self.name + '.weight', self.w, self.rw), (self.name + '.bias', self.b, self.rb)]


class _Norm:
    leaf = True

    def __init__(self, name, C, seed):
        self.name, self.C = name, C
        g, b = 1 + randn((C,), seed, 0.3), randn((C,), seed + 1000, 0.1)
        self.rg, self.rb = g.clone().requires_grad_(), b.clone().requires_grad_()
        self.g, self.b = _param(g), _param(b)

    def params(self):
        return [(self.name + '.gamma', self.g, self.rg), (self.name + '.beta', self.b, self.rb)]


class LN(_Norm):
    def gpu(self, x):
        from sid_lsg_amd import ops
        return ops.layer_norm(x, self.g, self.b, 1e-5)

    def ref(self, x):
        return F.layer_norm(x, (self.C,), self.rg, self.rb, 1e-5)


class GN(_Norm):
    """GroupNorm + SiLU of the first B * HW rows seen as [B, HW, C] (B = 2, HW = 64, 32 groups); the other rows end here."""
    B, HW, G = 2, 64, 32

    def gpu(self, x):
        from sid_lsg_amd import ops
        y = ops.group_norm(x[:self.B * self.HW].view(self.B, self.HW, self.C), self.g, self.b, self.G, 1e-5, True)
        return y.view(self.B * self.HW, self.C)

    def ref(self, x):
        xn = x[:self.B * self.HW].view(self.B, self.HW, self.C).permute(0, 2, 1)
        y = F.silu(F.group_norm(xn, self.G, self.rg, self.rb, 1e-5))
        return y.permute(0, 2, 1).reshape(self.B * self.HW, self.C)


class Seq:
    def __init__(self, *stages):
        self.stages = stages

    def gpu(self, x):
        for s in self.stages:
            x = tapped(s, x) if getattr(s, 'leaf', False) else s.gpu(x)
        return x

    def ref(self, x):
        for s in self.stages:
            x = s.ref(x)
        return x

    def leaf_uses(self):
        """How many ops the chain runs (a layer applied twice counts twice)."""
        return sum(1 if getattr(s, 'leaf', False) else s.leaf_uses() if isinstance(s, Seq) else 0 for s in self.stages)

    def params(self):
        out, seen = [], set()
        for s in self.stages:
            for p in s.params():
                if id(p[1]) not in seen:           # a layer applied twice is one set of parameters
                    seen.add(id(p[1]))
                    out.append(p)
        return out


class Checkpoint(Seq):
    """torch.utils.checkpoint around the stages; reentrant: the recomputed block runs its backward as a NESTED pass."""

    def __init__(self, reentrant, *stages):
        super().__init__(*stages)
        self.reentrant = reentrant

    def gpu(self, x):
        return checkpoint(lambda t: Seq.gpu(self, t), x, use_reentrant=self.reentrant)


class _Recompute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seq):
        ctx.seq = seq
        ctx.save_for_backward(x)
        return Seq.gpu(seq, x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        with torch.enable_grad():
            xi = x.detach().requires_grad_()
            y = Seq.gpu(ctx.seq, xi)
        (gx,) = torch.autograd.grad(y, xi, g)        # a nested pass; the ops accumulate their parameter gradients in place
        return gx, None


class InnerGrad(Seq):
    """The stages recomputed inside a Function.backward, their input gradient obtained with torch.autograd.grad."""

    def gpu(self, x):
        return _Recompute.apply(x, self)


class _Fail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError('injected host failure')


class _Stage:
    def ref(self, x):
        return x

    def params(self):
        return []


class Fail(_Stage):
    """Raises on the host in its backward (after everything downstream of it has run its backward)."""

    def gpu(self, x):
        return _Fail.apply(x)


class _Shift(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        buf = torch.empty(g.numel() + 8, device=g.device, dtype=g.dtype)
        v = buf[4:4 + g.numel()].view(g.shape)         # bf16: 8 bytes past a 16-byte boundary
        v.copy_(g)
        return v


class Shift(_Stage):
    """Identity whose backward hands on the gradient as a contiguous view that is NOT 16-byte aligned: the grouped weight-gradient
    queue refuses such an operand (ops._queue_dense_wgrad), the single entry point takes it (launch_wgrad: the bounds-checked
    register-staged kernel)."""

    def gpu(self, x):
        return _Shift.apply(x)


class Marker(_Stage):
    def __init__(self, cb):
        self.cb = cb

    def gpu(self, x):
        from sid_lsg_amd import ops
        return ops.grad_ready_marker(x, self.cb)


class Model(Seq):
    def zero(self):
        for _, p, _ in self.params():
            p.grad.zero_()

    def backward(self, x, dy_seed=7, input_grad=True):
        """One forward + backward of the HIP chain on the bf16 input x, with a random bf16 output gradient -> the run: what the taps
        recorded ('record', one entry per executed op) and the input leaf ('x')."""
        global _record
        run = {'record': [], 'x': x.to(DEV).requires_grad_(input_grad)}
        _record = run['record']
        try:
            y = self.gpu(run['x'])
            y.backward(randn(tuple(y.shape), dy_seed).to(BF16).to(DEV))
            torch.cuda.synchronize()
        finally:
            _record = None
        return run

    def check(self, run, what, stages=None, only=None):
        """The fp32 twin of every op that ran a backward (of `stages`: of those only), at the recorded tensors: the op's output and
        input gradient, then every parameter gradient (`only`: of those names) against the sum over the parameter's uses."""
        done = [e for e in run['record'] if 'dy' in e and (stages is None or e['stage'] in stages)]
        assert done, f'{what}: no op ran a backward'
        if stages is None and self.stages:
            # an op whose backward never ran would simply be missing from the comparison: every op of the chain must be there, once
            assert len(done) == self.leaf_uses(), f'{what}: {len(done)} ops ran a backward, the chain has {self.leaf_uses()}'
        params = Seq(*[e['stage'] for e in done]).params()
        for _, _, r in params:
            r.grad = None
        first_dx = None
        for i, e in enumerate(done):
            name = f'{what}: op {i} ({e["stage"].name})'
            xr = e['x'].float().cpu().requires_grad_('dx' in e)
            e['more_ref'] = [t.detach().float().cpu().requires_grad_() for t in e['more']]
            with torch.enable_grad():            # (a marker's callback runs inside a backward node: grad mode is off there)
                y = e['stage'].ref(xr, *e['more_ref'])
            y.backward(e['dy'].float().cpu())
            close(e['y'], y, TOL_BF16, name + ' output')
            if 'dx' in e:
                assert float(xr.grad.abs().max()) > 0, name
                close(e['dx'], xr.grad, TOL_BF16, name + ' input gradient')
                if first_dx is None and run['x'] is not None and e['x'].data_ptr() == run['x'].data_ptr():
                    first_dx = xr.grad
        for n, p, r in params:
            if only is not None and n not in only:
                continue
            assert r.grad is not None and float(r.grad.abs().max()) > 0, f'{what}: reference gradient of {n} is zero'
            got = p.grad.permute(0, 2, 3, 1).reshape(p.shape[0], -1) if p.grad.dim() == 4 else p.grad     # conv: [Cout, 9 Cin]
            close(got, r.grad, TOL_F32, f'{what}: {n}')
        if stages is None and run['x'] is not None and run['x'].requires_grad:
            assert first_dx is not None, f'{what}: the input gradient was never produced'
            close(run['x'].grad, first_dx, TOL_BF16, f'{what}: gradient of the chain input')
        return done


def assert_idle(what=''):
    """Nothing queued for a later launch: the weight-gradient queues, the set of queued dW, the kept workspaces and the library's own
    queue of every stream that deferred reductions."""
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    assert all(not q[1] for q in ops._wg_queues.values()), f'{what}: weight-gradient jobs left queued'
    assert not ops._wg_queued_dw, f'{what}: dW left marked as queued'
    assert all(not v[1] for v in ops._defer_streams.values()), f'{what}: partial-sum workspaces left'
    for h in ops._defer_streams:
        assert lib.sidlsg_pending_reductions.raw(h) in (-1, 0), f'{what}: reductions left queued in the library'


def x_in(M, C=320, seed=1):
    return randn((M, C), seed).to(BF16)


def nested_model(kind, shape='small'):
    """head -> nested block -> tail.  The backward runs the tail, then the block (as a nested pass), then the head: the outer pass
    queues work before AND after the nested one.
    small: 2 + 2 + 2 queued 128-tile jobs (< ops._WG_MAX: all still queued when the nested pass starts and ends);
    many:  6 + 3 + 5 (> _WG_MAX: a full group holding jobs of both passes is launched in the middle);
    wide:  M = 4096, 320 <-> 960: the 160 x 160-tile queue (ops._WG_MAX160 = 3) filled across the pass boundary."""
    def block(*stages):
        if kind == 'grad':
            return InnerGrad(*stages)
        return Checkpoint(kind == 'reentrant', *stages)
    if shape == 'wide':
        return Model(Lin('h0', 960, 320, 10), LN('hn', 960, 11), Lin('h1', 320, 960, 12),
                     block(Lin('b0', 960, 320, 20), LN('bn', 960, 21), Lin('b1', 320, 960, 22)),
                     Lin('t0', 960, 320, 30), Lin('t1', 320, 960, 31), LN('tn', 320, 32))
    if shape == 'many':
        head = [Lin(f'h{i}', 320, 320, 10 + i) for i in range(5)]
        tail = [Lin(f't{i}', 320, 320, 30 + i) for i in range(4)]
        return Model(*head[:2], LN('hn', 320, 18), *head[2:],
                     block(Lin('b0', 640, 320, 20), LN('bn', 640, 21), Lin('b1', 320, 640, 22), Lin('b2', 320, 320, 23)),
                     *tail, Lin('t4', 320, 320, 36), GN('tg', 320, 37), Lin('t5', 640, 320, 38))
    return Model(Lin('h0', 320, 320, 10), LN('hn', 320, 11), Lin('h1', 640, 320, 12),
                 block(Lin('b0', 320, 640, 20), LN('bn', 320, 21), Lin('b1', 320, 320, 22)),
                 Lin('t0', 320, 320, 30), GN('tg', 320, 31), Lin('t1', 640, 320, 32))


def shared_model(sub):
    """One Linear applied twice in a pass -> (model, input requires grad).
    a / c: both uses are queued (the second one to arrive first flushes the first);
    b: the use that runs its backward LAST gets an unaligned dY (Shift) -- refused by the queue, launched directly after the flush.  It
       is the first op of the chain and its input needs no gradient, so no GEMM ever reads the unaligned view."""
    L = Lin('shared', 320, 320, 40)
    if sub == 'b':
        return Model(L, Shift(), LN('n', 320, 41), L, Lin('out', 640, 320, 42)), False
    return Model(L, LN('n', 320, 41), L, Lin('out', 640, 320, 42)), True


def run_shared(sub, what):
    """Case 6 (and, in the worker, 7): the shared layer's gradient is the sum of both uses."""
    m, xgrad = shared_model(sub)
    if sub == 'c':
        for n, p, _ in m.params():
            if n.endswith('.weight'):
                p._grad_assign = True
                p.grad.fill_(float('nan'))
    run = m.backward(x_in(512, seed=3), input_grad=xgrad)
    done = m.check(run, what)
    assert sum(e['stage'].name == 'shared' for e in done) == 2, 'both uses ran their backward'
    assert_idle(what)
    return m
