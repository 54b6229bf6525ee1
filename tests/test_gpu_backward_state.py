"""Backward-pass bookkeeping of sid_lsg_amd/ops.py under nested and failed backward passes.

ops.py keeps grouped weight-gradient jobs, deferred dgamma / dbeta reductions and shared column-gradient buffers alive across the
nodes of one backward pass (the ledger ops._passes, sid_lsg_amd/backward_state.py).  Every case here builds a small chain of the
project's own ops, computes the same chain in fp32 on the CPU with torch autograd -- op by op at the bf16 tensors the HIP chain
stored, see tests/backward_state_cases.py for why -- and compares every parameter gradient and the input gradient: 2e-3 of max|ref|
for the fp32 parameter gradients, 1.2e-2 for bf16 tensors, after asserting that the reference gradient is not zero -- a dropped or
doubled contribution is an error of the size of the gradient.
Every failure injected here is a Python exception raised on the host.
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import backward_state_cases as bc
from backward_state_cases import BF16, DEV, Checkpoint, Fail, GN, LN, Lin, Marker, Model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()   # fail loudly if the HIP library is missing
    from sid_lsg_amd import ops
    assert ops._WG_GROUP and ops._DEFER and ops._WG_MAX == 8 and ops._WG_MAX160 == 3, 'the cases are sized for the default queues'
    return ops


def M_of(shape):
    return 4096 if shape == 'wide' else 512


# ---- cases 1 - 3: a nested pass in the middle of the outer one ---------------------------------------------------------------------
@pytest.mark.parametrize('shape', ['small', 'many', 'wide'])
@pytest.mark.parametrize('kind', ['reentrant', 'grad', 'nonreentrant'])
def test_nested_pass_keeps_the_outer_gradients(ops, kind, shape):
    """reentrant: torch.utils.checkpoint(use_reentrant=True); grad: torch.autograd.grad inside a Function.backward -- both run the
    block's backward as a pass with a graph-task id of its own while the outer pass is live.  nonreentrant: the recomputation runs
    inside the outer task (forward ops while a backward pass is live).  Outer and inner gradients equal the reference and nothing
    stays queued."""
    m = bc.nested_model(kind, shape)
    what = f'{kind} / {shape}'
    m.check(m.backward(bc.x_in(M_of(shape))), what)
    bc.assert_idle(what)


# ---- case 4: a pass that raises, then a clean pass -----------------------------------------------------------------------------------
def failing_layers(n_lin):
    if n_lin <= 4:
        return [Lin('l0', 320, 320, 50), LN('n0', 320, 51), Lin('l1', 640, 320, 52), Lin('l2', 320, 640, 53), GN('g0', 320, 54),
                Lin('l3', 320, 320, 55)]
    return [Lin(f'l{i}', 320, 320, 50 + i) for i in range(n_lin // 2)] + [LN('n0', 320, 70)] + \
           [Lin(f'l{i}', 320, 320, 50 + i) for i in range(n_lin // 2, n_lin)]


def run_failing(bad, x):
    with pytest.raises(RuntimeError, match='injected host failure'):
        bad.backward(x, dy_seed=9)
    torch.cuda.synchronize()


@pytest.mark.parametrize('n_lin', [4, 10])
def test_failed_pass_then_clean_pass_after_zeroing(ops, n_lin):
    """(a) The failure fires upstream of every layer, with weight-gradient jobs and norm reductions queued and unflushed (n_lin = 10:
    more than _WG_MAX, one full group was already launched).  After zeroing, a clean pass on OTHER inputs leaves exactly its own
    gradients: nothing of the dead pass is launched into them."""
    layers = failing_layers(n_lin)
    run_failing(Model(Fail(), *layers), bc.x_in(512, seed=5))
    good = Model(*layers)
    good.zero()
    good.check(good.backward(bc.x_in(512, seed=6)), f'clean pass after a failed one ({n_lin} Linear)')
    bc.assert_idle('after the clean pass')


def test_dropped_job_gives_its_assign_mark_back(ops):
    """(b) The state optim.FusedAdamEMA leaves, made visible: `_grad_assign` set and .grad full of NaN on the weights.  The failing
    pass takes the marks when it queues the jobs; the jobs are dropped.  Without zeroing, the clean pass must still OVERWRITE: every
    weight whose job was dropped holds exactly the clean pass's gradient, finite."""
    layers = failing_layers(4)
    good = Model(*layers)
    weights = [p for n, p, _ in good.params() if n.endswith('.weight')]
    for p in weights:
        p._grad_assign = True
        p.grad.fill_(float('nan'))
    run_failing(Model(Fail(), *layers), bc.x_in(512, seed=5))
    # (only those: the GroupNorm of this size adds its dgamma / dbeta without a deferred reduction -- gradients the dead pass has
    # WRITTEN stay the caller's to zero, as in plain PyTorch)
    good.check(good.backward(bc.x_in(512, seed=6)), 'assign mark after a dropped job', only=[n for n, _, _ in good.params() if n.endswith('.weight')])
    assert not any(getattr(p, '_grad_assign', False) for p in weights), 'the clean pass takes the marks'
    bc.assert_idle()


# ---- case 5: the stale-state cleanup and the nesting rule together ---------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['reentrant', 'grad'])
def test_failed_pass_then_nested_pass(ops, kind):
    m = bc.nested_model(kind)
    run_failing(Model(Fail(), *m.stages), bc.x_in(512, seed=5))
    m.zero()
    m.check(m.backward(bc.x_in(512, seed=6)), f'{kind} pass after a failed one')
    bc.assert_idle('after the nested pass')


def test_failure_inside_a_nested_pass(ops):
    """The block's backward -- a nested pass -- raises after queuing its jobs, with the outer tail's jobs queued as well: both passes
    die.  Then a clean nested pass over the same layers."""
    head = [Lin('h0', 320, 320, 10), LN('hn', 320, 11), Lin('h1', 640, 320, 12)]
    block = [Lin('b0', 320, 640, 20), LN('bn', 320, 21), Lin('b1', 320, 320, 22)]
    tail = [Lin('t0', 320, 320, 30), GN('tg', 320, 31), Lin('t1', 640, 320, 32)]
    run_failing(Model(*head, Checkpoint(True, Fail(), *block), *tail), bc.x_in(512, seed=5))
    bc.assert_idle('after the failed nested pass')
    m = Model(*head, Checkpoint(True, *block), *tail)
    m.zero()
    m.check(m.backward(bc.x_in(512, seed=6)), 'nested pass after a failure inside a nested pass')
    bc.assert_idle('after the clean pass')


# ---- cases 6, 7: a layer applied twice in one pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('sub', ['a', 'b', 'c'])
def test_shared_layer_sums_both_uses(ops, sub):
    """a: both uses are queued; b: one is queued, the other is refused by the queue (dY not 16-byte aligned) and launched directly;
    c: `_grad_assign` set and .grad NaN -- the first use assigns, the second accumulates."""
    bc.run_shared(sub, f'shared layer ({sub})')


def test_shared_layer_with_two_weight_gradient_streams(ops):
    """SIDLSG_WGRAD_STREAMS is read when ops.py is imported: tests/backward_state_worker.py runs the three shared-layer cases with two
    round-robin weight-gradient streams in a fresh process and asserts from ops.wgrad_order_log that two launches on one dW either
    share a stream or have a wait_stream between them (values alone cannot prove the absence of a race)."""
    env = dict(os.environ, SIDLSG_WGRAD_STREAMS='2')
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'backward_state_worker.py')], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and 'shared dW ordered on two streams: ok' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- case 8: a gradient-ready marker in the middle of the chain --------------------------------------------------------------------------
@pytest.mark.parametrize('nested', [False, True])
def test_marker_sees_final_gradients_behind_it(ops, nested):
    """When the marker's callback fires, the gradients of everything behind it (here: the block and the tail) are complete -- compared
    inside the callback, after a device sync -- and the head's are still untouched."""
    head = [Lin('h0', 320, 320, 10), LN('hn', 320, 11), Lin('h1', 640, 320, 12)]
    block = [Lin('b0', 320, 640, 20), LN('bn', 320, 21), Lin('b1', 320, 320, 22)]
    tail = [Lin('t0', 320, 320, 30), GN('tg', 320, 31), Lin('t1', 640, 320, 32)]
    fired = []

    def cb():
        torch.cuda.synchronize()
        done = Model().check({'record': bc._record, 'x': None}, f'at the marker (nested={nested})', stages=set(block + tail))
        assert len(done) == 6, 'block and tail have run their backward'
        for n, p, _ in Model(*head).params():
            assert float(p.grad.abs().max()) == 0.0, f'{n}: written before its node ran'
        fired.append(True)
    m = Model(*head, Marker(cb), Checkpoint(True, *block) if nested else bc.Seq(*block), *tail)
    run = m.backward(bc.x_in(512))
    assert fired == [True]
    m.check(run, f'marker (nested={nested})')
    bc.assert_idle()


# ---- case 9: the shared column-gradient buffer -----------------------------------------------------------------------------------------
class ConvRV:
    """3x3 conv C -> C whose output gets a per-sample row vector added: a column slice of a split_columns() source, so the row
    vector's gradient is accumulated into the shared column-gradient buffer (ops.colsum(slot=...))."""

    def __init__(self, ops, name, C, seed):
        self.name, self.C = name, C
        w = (bc.randn((C, 9 * C), seed) * (9 * C) ** -0.5).to(BF16)
        b = bc.randn((C,), seed + 1000, 0.1)
        self.rw, self.rb = w.float().requires_grad_(), b.clone().requires_grad_()
        self.w = torch.nn.Parameter(w.float().view(C, 3, 3, C).permute(0, 3, 1, 2).to(DEV))     # logical [Cout, Cin, 3, 3], channels-last storage
        self.w.grad = torch.zeros(C, 3, 3, C, device=DEV).permute(0, 3, 1, 2)
        self.b = torch.nn.Parameter(b.to(DEV))
        self.b.grad = torch.zeros_like(self.b)
        self.w16 = w.to(DEV)
        self.w16t = ops.transpose_w(self.w.permute(0, 2, 3, 1), C, C, 9)
        self.ops = ops

    def params(self):
        return [(self.name + '.weight', self.w, self.rw), (self.name + '.bias', self.b, self.rb)]

    def gpu(self, x, part):
        return self.ops.conv3x3_op(x, self.w, self.b, self.w16, self.w16t, None, part, 1, 0, False)

    def ref(self, x, part):
        wn = self.rw.view(self.C, 3, 3, self.C).permute(0, 3, 1, 2)
        y = F.conv2d(x.permute(0, 3, 1, 2), wn, padding=1).permute(0, 2, 3, 1)
        return y + self.rb + part[:, None, None, :]


@pytest.mark.parametrize('after_failure', [False, True])
def test_column_gradients_across_a_nested_pass(ops, after_failure):
    """Two consumers of one split_columns() source sit on both sides of a re-entrant checkpoint: the source's gradient -- built in the
    shared buffer by both -- the conv and the block gradients equal the reference; also as the clean pass after a failed one, whose
    own half-built buffer must have gone with it."""
    B, H, C = 2, 8, 320
    ca, cb = ConvRV(ops, 'conv_a', C, 60), ConvRV(ops, 'conv_b', C, 62)
    block = Checkpoint(True, Lin('b0', 320, 320, 64), LN('bn', 320, 65), Lin('b1', 320, 320, 66))

    holders = []

    def gpu(x, emb, fail=False):
        p0, p1 = ops.split_columns(emb, [C, C])
        holders.append(p0._col_slot[0])
        h = bc.tapped(ca, bc._Fail.apply(x) if fail else x, p0)
        h = block.gpu(h.view(B * H * H, C)).view(B, H, H, C)
        return bc.tapped(cb, h, p1)

    def run(seed, fail=False):
        x, emb = bc.randn((B, H, H, C), seed).to(BF16), bc.randn((B, 2 * C), seed + 1)
        dy = bc.randn((B, H, H, C), seed + 2).to(BF16).to(DEV)
        r = {'record': [], 'x': x.to(DEV).requires_grad_()}
        ed = emb.to(DEV).requires_grad_()
        bc._record = r['record']
        try:
            if fail:
                with pytest.raises(RuntimeError, match='injected host failure'):
                    gpu(r['x'], ed, True).backward(dy)
            else:
                gpu(r['x'], ed).backward(dy)
            torch.cuda.synchronize()
        finally:
            bc._record = None
        if fail:
            # conv_b ran its backward, so its row-vector gradient went into the holder's buffer; the pass then died with the buffer
            # not yet taken (_SplitColumns.backward never ran): the buffer is dropped with the pass
            assert 'dx' in next(e for e in r['record'] if e['stage'] is cb)
            assert holders[-1].buf is None, 'the column-gradient buffer of a dead pass is still there'
            return
        assert holders[-1].buf is None, 'the buffer was handed on by _SplitColumns.backward'
        done = Model().check(r, f'column gradients (after a failure: {after_failure})')
        assert [e['stage'].name for e in done] == ['conv_a', 'conv_b', 'b0', 'bn', 'b1']
        eref = torch.cat([e['more_ref'][0].grad for e in done[:2]], dim=1)
        assert float(eref.abs().max()) > 0
        bc.close(ed.grad, eref, bc.TOL_F32, 'split_columns source gradient')
        bc.assert_idle()

    if after_failure:
        run(70, fail=True)
        bc.assert_idle('after the failed pass')
        for p in (ca.w, ca.b, cb.w, cb.b, *[p for _, p, _ in block.params()]):
            p.grad.zero_()
    run(80)
