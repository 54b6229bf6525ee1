"""Which backward pass owns what: the bookkeeping behind the queues that ops.py keeps alive across the nodes of one backward pass
(grouped weight-gradient jobs, deferred dgamma / dbeta reductions, the shared column-gradient buffers, the weight-gradient join).

Needs torch's autograd engine only -- no device, no library -- so that it can be tested with CPU tensors (tests/test_backward_state_host.py).

The contract:
  * an entry is tagged with the graph-task id of the pass that queued it (torch._C._current_graph_task_id());
  * a pass is LIVE from its first entry until the engine callback it queued then has run.  Several passes can be live at once: a
    re-entrant pass (torch.utils.checkpoint(use_reentrant=True), autograd.grad or backward inside a Function.backward) has its own
    id and ends, callback included, while the pass that started it is still running;
  * when a live pass ends, everything queued is launched -- the entries of the other live passes too: an entry is complete work the
    moment it is queued, so launching an outer pass's entries early is harmless; each entry is launched exactly once;
  * a pass that RAISED never runs its callbacks: the engine frees them with the graph task.  "Callback freed without having run" is
    therefore what a dead pass looks like, and at that moment its entries -- and only its own -- are handed to `drop`, never to
    `launch`.  WHEN that moment is: the graph task goes with its last reference.  If the backward ran on the calling thread (CPU
    nodes) that is before backward() raises.  With device nodes the engine's worker thread of the device may hold the last reference
    a little longer than the caller, which the exception has already woken: the drop then runs ON THAT WORKER THREAD, possibly just
    after backward() has raised -- but before that thread takes up a node of any later pass on the device, which is what the
    contract needs (a later pass never sees, flushes or launches a dead entry).  Code that inspects the queues right after a failed
    backward() must let the worker get there first (the tests synchronise the device and then read).  Every method takes the
    ledger's lock, and the hooks run under it, so the worker thread's drop and the caller's thread cannot interleave;
  * outside a backward pass (id < 0) nothing can be queued: add() launches right away.
"""
import functools
import threading
import weakref

import torch


class _Token:
    """Lives exactly as long as the engine holds the end-of-pass callback of one pass."""
    __slots__ = ('__weakref__',)


def _engine_task_id():
    return torch._C._current_graph_task_id()


def _engine_queue_callback(fn):
    torch.autograd.Variable._execution_engine.queue_callback(fn)


def _locked(fn):
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        with self._lock:
            return fn(self, *args, **kwargs)
    return wrapper


class PassLedger:
    """launch(key, entries): run the entries of one queue (in the order they were queued); drop(key, entries): forget them (their pass
    raised).  task_id / queue_callback: the engine's, replaceable in tests."""

    def __init__(self, launch, drop, task_id=_engine_task_id, queue_callback=_engine_queue_callback):
        self._launch, self._drop = launch, drop
        self._task_id, self._queue_callback = task_id, queue_callback
        self._queues = {}        # key -> [(task id, entry)], the list object is never replaced (ops.py hands it out)
        self._live = {}          # task id -> finalizer of the pass's token
        self._once = {}          # task id -> marks taken by once()
        self._undo = {}          # task id -> functions to call if the pass dies (on_death)
        self._lock = threading.RLock()   # a dead pass is dropped on whichever thread lets go of it last (see the module docstring)

    # ---- passes ----
    def current(self):
        return self._task_id()

    @_locked
    def is_live(self, tid):
        return tid in self._live

    @_locked
    def live(self):
        return sorted(self._live)

    @_locked
    def arm(self):
        """Make the current pass live (first call of the pass: queues its end-of-pass callback).  -> its id (< 0: no pass)."""
        tid = self._task_id()
        if tid < 0 or tid in self._live:
            return tid
        token = _Token()

        def done():
            try:
                self.flush()                 # the pass is still live here: a launch hook may ask once() or queue callbacks of its own
            finally:
                self._end(tid, token)
        fin = weakref.finalize(token, self._died, tid)       # holds no reference to the token: runs when the engine lets go of `done`
        fin.atexit = False
        self._live[tid] = fin
        self._queue_callback(done)
        return tid

    @_locked
    def _end(self, tid, token):
        fin = self._live.pop(tid, None)
        if fin is not None:
            fin.detach()
        self._once.pop(tid, None)
        self._undo.pop(tid, None)

    @_locked
    def _died(self, tid):
        self._live.pop(tid, None)
        self._once.pop(tid, None)
        for fn in self._undo.pop(tid, ()):
            fn()
        for key, q in self._queues.items():
            dead = [e for t, e in q if t == tid]
            if dead:
                q[:] = [(t, e) for t, e in q if t != tid]
                self._drop(key, dead)

    @_locked
    def once(self, mark):
        """True the first time `mark` is asked for in the current pass (which becomes live); always True outside a pass."""
        tid = self.arm()
        if tid < 0:
            return True
        marks = self._once.setdefault(tid, set())
        if mark in marks:
            return False
        marks.add(mark)
        return True

    @_locked
    def on_death(self, fn):
        """Call fn() if the current pass raises (never if it ends well); nothing to undo outside a pass."""
        tid = self.arm()
        if tid >= 0:
            self._undo.setdefault(tid, []).append(fn)

    # ---- entries ----
    @_locked
    def queue(self, key):
        """The list of (task id, entry) of `key`: read it, never write it."""
        return self._queues.setdefault(key, [])

    @_locked
    def owners(self, key):
        return {t for t, _ in self._queues.get(key, ())}

    @_locked
    def pending(self):
        return sum(len(q) for q in self._queues.values())

    @_locked
    def add(self, key, entry):
        """Queue `entry` for the current pass; outside a pass it is launched right away (behind whatever `key` still holds)."""
        tid = self.arm()
        self.queue(key).append((tid, entry))
        if tid < 0:
            self.flush(key)
        return tid

    @_locked
    def flush(self, key=None):
        """Launch what is queued under `key` (None: under every key).  The queue is emptied BEFORE the hook runs, so that an entry is
        launched once even if the hook raises or queues again."""
        for k in ([key] if key is not None else list(self._queues)):
            q = self._queues.get(k)
            if q:
                entries = [e for _, e in q]
                del q[:]
                self._launch(k, entries)
