"""The bookkeeping of backward passes (sid_lsg_amd/backward_state.py: PassLedger) with CPU tensors and torch's own autograd engine:
no device, no library.  CPU autograd Functions stand in for the ops: like ops._Linear.backward they take their parameter's `assign`
mark, queue one entry per node and flush a queue that is full; the launch / drop hooks only record.

What is pinned: a re-entrant nested pass does not drop the outer pass's entries; each entry is launched exactly once; a pass that
raised has its entries dropped, never launched, and its marks returned; nothing is left behind; outside a pass add() launches at once.
"""
import pytest
import torch
from torch.utils.checkpoint import checkpoint

from sid_lsg_amd.backward_state import PassLedger

QMAX = 4          # stands for ops._WG_MAX


class Param:
    def __init__(self, name, assign=False):
        self.name, self._grad_assign = name, assign


class Book:
    """A ledger with recording hooks, as ops.py wires it (_launch_entries / _drop_entries)."""

    def __init__(self):
        self.launched, self.dropped, self.tids, self.groups = [], [], {}, []
        self.led = PassLedger(self._launch, self._drop)

    def _launch(self, key, entries):
        self.groups.append((key, [p.name for p, _ in entries]))
        self.launched += [p.name for p, _ in entries]

    def _drop(self, key, entries):
        for p, assign in entries:
            self.dropped.append(p.name)
            if assign:
                p._grad_assign = True

    def idle(self):
        return self.led.pending() == 0 and self.led.live() == [] and not self.led._once and not self.led._undo


class Op(torch.autograd.Function):
    """y = 2 x; the backward queues one entry for `param` under `key`."""

    @staticmethod
    def forward(ctx, x, book, param, key):
        ctx.a = (book, param, key)
        return x * 2

    @staticmethod
    def backward(ctx, g):
        book, param, key = ctx.a
        assign, param._grad_assign = param._grad_assign, False
        tid = book.led.add(key, (param, assign))
        book.tids[param.name] = tid
        if len(book.led.queue(key)) >= QMAX:
            book.led.flush(key)
        return g * 2, None, None, None


class Fail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError('injected failure')


class InnerGrad(torch.autograd.Function):
    """Recomputes Op(param) under enable_grad in its backward and runs torch.autograd.grad there: a nested pass.  swallow: an inner
    failure is caught and a zero gradient returned (the outer pass lives on)."""

    @staticmethod
    def forward(ctx, x, book, param, key, fail, swallow):
        ctx.a = (book, param, key, fail, swallow)
        ctx.save_for_backward(x)
        return x * 2

    @staticmethod
    def backward(ctx, g):
        book, param, key, fail, swallow = ctx.a
        (x,) = ctx.saved_tensors
        with torch.enable_grad():
            xi = x.detach().requires_grad_()
            y = Op.apply(Fail.apply(xi) if fail else xi, book, param, key)
        try:
            (gx,) = torch.autograd.grad(y, xi, g)
        except RuntimeError:
            if not swallow:
                raise
            gx = torch.zeros_like(g)
        return gx, None, None, None, None, None


def chain(book, names, x, key='q', assign=False):
    params = [Param(n, assign) for n in names]
    for p in params:
        x = Op.apply(x, book, p, key)
    return x, params


def leaf():
    return torch.ones(3, requires_grad=True)


def test_plain_pass_launches_everything_once_at_the_end():
    book = Book()
    x = leaf()
    y, _ = chain(book, 'abc', x)
    y.sum().backward()
    assert book.launched == ['c', 'b', 'a'] and book.dropped == [] and book.groups == [('q', ['c', 'b', 'a'])]
    assert torch.equal(x.grad, torch.full((3,), 8.0))
    assert book.idle()


def test_full_queue_is_launched_before_the_end_and_nothing_twice():
    book = Book()
    y, _ = chain(book, 'abcdef', leaf())
    y.sum().backward()
    assert book.groups == [('q', ['f', 'e', 'd', 'c']), ('q', ['b', 'a'])]
    assert sorted(book.launched) == list('abcdef') and book.idle()


@pytest.mark.parametrize('nested', ['checkpoint', 'autograd.grad'])
def test_reentrant_nested_pass_keeps_the_outer_entries(nested):
    book = Book()
    x = leaf()
    h, _ = chain(book, 'ab', x)
    if nested == 'checkpoint':
        inner = [Param('i1'), Param('i2')]
        h = checkpoint(lambda t: Op.apply(Op.apply(t, book, inner[0], 'q'), book, inner[1], 'q'), h, use_reentrant=True)
        scale = 2.0 ** 6
    else:
        h = InnerGrad.apply(h, book, Param('i1'), 'q', False, False)
        scale = 2.0 ** 5
    y, _ = chain(book, 'cd', h, key='r')
    y.sum().backward()
    names = sorted(book.tids)
    assert sorted(book.launched) == names, 'every entry exactly once'
    assert book.dropped == []
    outer = {book.tids[n] for n in 'abcd'}
    assert len(outer) == 1 and book.tids['i1'] not in outer, 'the nested pass has a graph-task id of its own'
    assert torch.equal(x.grad, torch.full((3,), scale))
    assert book.idle()


def test_failed_pass_drops_its_entries_and_returns_their_marks():
    book = Book()
    x = leaf()
    y, params = chain(book, 'abc', Fail.apply(x), assign=True)
    with pytest.raises(RuntimeError, match='injected failure'):
        y.sum().backward()
    assert book.launched == [] and sorted(book.dropped) == ['a', 'b', 'c']
    assert all(p._grad_assign for p in params), 'a dropped entry gives its mark back'
    assert book.idle()
    # the next, clean pass is its own: nothing of the dead one is launched into it
    y, _ = chain(book, 'de', leaf())
    y.sum().backward()
    assert book.launched == ['e', 'd'] and sorted(book.dropped) == ['a', 'b', 'c'] and book.idle()


def test_failed_pass_with_a_full_queue_keeps_what_was_launched_and_drops_the_rest():
    book = Book()
    y, params = chain(book, 'abcdef', Fail.apply(leaf()), assign=True)
    with pytest.raises(RuntimeError):
        y.sum().backward()
    assert book.launched == ['f', 'e', 'd', 'c'] and sorted(book.dropped) == ['a', 'b']
    assert [p._grad_assign for p in params] == [True, True, False, False, False, False]
    assert book.idle()


def test_failed_pass_then_nested_pass():
    book = Book()
    y, _ = chain(book, 'ab', Fail.apply(leaf()))
    with pytest.raises(RuntimeError):
        y.sum().backward()
    x = leaf()
    h, _ = chain(book, 'c', x)
    h = InnerGrad.apply(h, book, Param('i'), 'q', False, False)
    y, _ = chain(book, 'd', h)
    y.sum().backward()
    assert sorted(book.dropped) == ['a', 'b'] and sorted(book.launched) == ['c', 'd', 'i']
    assert torch.equal(x.grad, torch.full((3,), 8.0)) and book.idle()


def test_failure_inside_a_nested_pass_takes_both_passes_down():
    book = Book()
    h, _ = chain(book, 'a', leaf())
    h = InnerGrad.apply(h, book, Param('i', True), 'q', True, False)
    y, _ = chain(book, 'b', h)
    with pytest.raises(RuntimeError, match='injected failure'):
        y.sum().backward()
    assert book.launched == [] and sorted(book.dropped) == ['b', 'i']       # 'a' is upstream of the failure: never reached
    assert book.idle()


def test_failure_inside_a_nested_pass_that_the_outer_pass_survives():
    """Only the dead pass's entries go: the outer pass's, queued before and after, are launched."""
    book = Book()
    x = leaf()
    h, _ = chain(book, 'a', x)
    inner = Param('i', True)
    h = InnerGrad.apply(h, book, inner, 'q', True, True)
    y, _ = chain(book, 'b', h)
    y.sum().backward()
    assert book.dropped == ['i'] and inner._grad_assign
    assert sorted(book.launched) == ['a', 'b'] and book.idle()


def test_outside_a_backward_pass_entries_launch_right_away():
    book = Book()
    assert book.led.current() < 0 and book.led.arm() < 0
    p = Param('now')
    assert book.led.add('q', (p, False)) < 0
    assert book.launched == ['now'] and book.idle()
    assert book.led.once('mark') and book.led.once('mark'), 'no pass: nothing to remember'
    book.led.on_death(lambda: book.dropped.append('never'))
    assert book.dropped == [] and book.idle()


def test_once_marks_and_death_hooks_live_with_their_pass():
    book = Book()
    seen = []

    class Mark(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, fail_hook):
            ctx.h = fail_hook
            return x * 1

        @staticmethod
        def backward(ctx, g):
            seen.append(book.led.once('join'))
            book.led.on_death(lambda: seen.append(ctx.h))
            return g, None

    x = leaf()
    Mark.apply(Mark.apply(x, 'no'), 'no').sum().backward()
    assert seen == [True, False] and book.idle()
    del seen[:]
    with pytest.raises(RuntimeError):
        Mark.apply(Mark.apply(Fail.apply(x), 'died'), 'died').sum().backward()
    assert seen == [True, False, 'died', 'died'] and book.idle()
    del seen[:]
    Mark.apply(x, 'no').sum().backward()
    assert seen == [True] and book.idle()
