"""Host side of the HIP kernels: thin launch wrappers + torch.autograd.Function glue.

Follows the reference's op-wrapper convention (torch_utils/ops/bias_act.py: public function ->
cached autograd.Function -> plugin call on the current stream) with one deliberate difference:
there is no `impl='ref'` fallback.  If the library is absent or a tensor is not on the GPU these
raise.  PyTorch is used only for device memory, the current stream and autograd bookkeeping.

Conventions: activations are bf16 (production) or fp32 (the fp32-accurate parity mode: same call graph, the `_f32`
entry-point family of include/sidlsg_hip.h, chosen by the dtype of the activation tensor), NHWC / token-major and
contiguous; parameters are fp32
"masters" whose `.grad` is a pre-allocated fp32 view into the network's flat gradient buffer --
weight/bias gradients are ACCUMULATED IN PLACE by the kernels (atomics / +=) and the autograd
functions return None for them, so no per-parameter gradient tensors are ever materialised.
"""
import contextlib
import ctypes
import functools
import weakref
import os

import torch

from ._lib import lib
from .backward_state import PassLedger
from .scheduler import prediction_mode

BF16 = torch.bfloat16
F32 = torch.float32


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


ACT = 'act'   # _chk: an activation tensor (bf16 or fp32)


def _chk(t, dtype=None):
    if not t.is_cuda:
        raise RuntimeError('sid_lsg_amd ops need CUDA(HIP) tensors: there is no CPU fallback')
    if dtype is ACT:
        if t.dtype not in (BF16, F32):
            raise RuntimeError(f'expected a bf16 or fp32 activation tensor, got {t.dtype}')
    elif dtype is not None and t.dtype != dtype:
        raise RuntimeError(f'expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise RuntimeError('expected a contiguous tensor')
    return t


def _fn(name, dtype, bf16_suffix=''):
    """C entry point of the activation dtype: `sidlsg_<name><bf16_suffix>` for bf16, `sidlsg_<name>_f32` for fp32."""
    return getattr(lib, f'sidlsg_{name}_f32' if dtype == F32 else f'sidlsg_{name}{bf16_suffix}')


def _wants_grad(p):
    """Weight gradients are wanted iff the parameter requires grad.  Its `.grad` is the pre-bound view of the network's flat
    gradient buffer: HipUNet2DCondition re-binds (and zeroes) the views at the start of every forward if a foreign optimizer
    ran `zero_grad(set_to_none=True)` (sid_training_loop.py:390,469); a None that appears between a forward and its backward
    is re-bound here the same way."""
    if p is None or not p.requires_grad:
        return False
    if p.grad is None:
        # zero_grad(set_to_none=True) between a forward and its backward (a retained graph, an accumulation round of a
        # foreign optimizer): None means zero to the caller, so the flat-buffer view comes back zeroed
        flat = getattr(p, '_flat_grad', None)
        if flat is None:
            raise RuntimeError('parameter requires grad but has no gradient buffer to bind (not a HipUNet2DCondition parameter?): '
                               'weight gradients would be lost')
        flat.zero_()
        p.grad = flat
    return True


def _take_assign(weight, dtype):
    """True when this weight gradient may OVERWRITE `weight.grad`: the fused optimizer left the view un-zeroed after its last step
    and marked the parameter (`_grad_assign`, optim.FusedAdamEMA with a network that has an assign plan); the first weight gradient
    after that step takes the mark.  Saves the optimizer's zero stores and the read of dW here (sidlsg_*wgrad_assign_bf16: bit-identical
    to accumulating onto zeros).  A launch that cannot overwrite (fp32 activations) zeroes the view instead and accumulates."""
    if not getattr(weight, '_grad_assign', False):
        return False
    weight._grad_assign = False
    if dtype != BF16:
        weight.grad.zero_()
        return False
    return True



# ------------------------------------------------------------------------------------------------
_workspace = {}


def _dev_key(device):
    """Cache key of a device: its index; an index-less 'cuda' device means the CURRENT device (not device 0)."""
    idx = torch.device(device).index
    return torch.cuda.current_device() if idx is None else idx


def ensure_workspace(device, nbytes=512 << 20):
    """fp32 split-K scratch for the small-pixel-count convs/GEMMs (allocated once per device through torch's allocator)."""
    key = _dev_key(device)
    if key not in _workspace:
        ws = torch.empty(nbytes // 4, device=device, dtype=F32)
        lib.sidlsg_set_workspace(ws.data_ptr(), ws.numel() * 4)
        _workspace[key] = ws
    return _workspace[key]


_stream_ws = {}
_side_streams = {}


def side_stream(device):
    """The process-wide second compute stream of `device` (with its private split-K workspace): created once, shared by
    every SiDStep -- the C library keeps at most 4 stream workspaces."""
    key = _dev_key(device)
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
        ensure_stream_workspace(_side_streams[key])
    return _side_streams[key]


# ---- deterministic mode ---------------------------------------------------------------------------------------------------------
# include/sidlsg_hip.h sidlsg_set_deterministic: every parameter-gradient reduction of the library in an order-fixed form.  On the host
# side the mode also keeps the weight gradients on ONE side stream (wgrad_stream) and the optimizer steps after the whole backward
# (sid_step.py: no segment-wise updates).  Policy: an explicit set_deterministic(True / False) wins; None (the default) = on when
# SIDLSG_DETERMINISTIC is a non-zero integer, else what torch.use_deterministic_algorithms() says.  sync_deterministic() writes the
# effective value to the library; every backward of this module calls it first, so a caller who only sets the torch flag and then
# runs loss.backward() gets the deterministic kernels.
def _env_int(name):
    try:
        return int(os.environ.get(name, '0').strip() or '0')
    except ValueError:
        return 0


_det_explicit = None
_det_env = _env_int('SIDLSG_DETERMINISTIC') != 0
_det_lib = None            # the value last written to the library


def is_deterministic():
    """The effective mode (see set_deterministic)."""
    if _det_explicit is not None:
        return _det_explicit
    return _det_env or torch.are_deterministic_algorithms_enabled()


def sync_deterministic():
    """Write the effective mode to the library's process-wide flag (when it changed); returns it."""
    global _det_lib
    on = is_deterministic()
    if on != _det_lib:
        lib.sidlsg_set_deterministic.raw(1 if on else 0)
        _det_lib = on
    return on


def set_deterministic(mode):
    """mode: True / False = on / off whatever the environment says; None = follow SIDLSG_DETERMINISTIC, then the torch flag.
    Returns the effective mode.  A captured graph keeps the kernels of the mode it was captured in."""
    global _det_explicit
    if mode is not True and mode is not False and mode is not None:
        raise ValueError(f'set_deterministic: expected True, False or None, got {mode!r}')
    _det_explicit = mode
    return sync_deterministic()


@contextlib.contextmanager
def deterministic(mode=True):
    """with ops.deterministic(): ... -- set_deterministic(mode) for the block, the previous setting restored after it."""
    old = _det_explicit
    set_deterministic(mode)
    try:
        yield
    finally:
        set_deterministic(old)


# ---- weight gradients on their own stream ---------------------------------------------------------------------------------
# A weight-gradient launch is one round of equal-work blocks: they start together, wait for their tile DMAs together and end in
# a chip-wide burst of slab writes followed by a small reduction kernel (tools/ab/wgrad_trace.py) -- MFMA and HBM idle in
# turns.  dW of a layer depends only on (dY, saved x), not on the backward-data chain, so these launches go to a second stream
# and their idle phases are filled by the dgrad GEMMs / attention / norm kernels of the main stream (and vice versa).
# Ordering: the side stream waits for the main stream at each launch (dY exists), the tensors are record_stream()-ed, and
# the main stream (plus, through grad_streams(), the gradient-exchange stream) waits for the side stream at the end of the
# backward pass (autograd engine callback), i.e. before anything may read .grad.  SIDLSG_WGRAD_STREAM=0 turns it off.
_WGRAD_SIDE = os.environ.get('SIDLSG_WGRAD_STREAM', '1') != '0'
# SIDLSG_WGRAD_STREAMS = n > 1: weight-gradient launches rotate over n streams, so that n of them can share the chip (with
# SIDLSG_WGRAD_SLOTS = 512 / n each launch splits its pixel range for 1 / n of the chip: fewer, longer blocks and 1 / n of the
# partial-sum slab traffic per layer).  A/B knob; default 1.
_WGRAD_NSTREAMS = max(1, int(os.environ.get('SIDLSG_WGRAD_STREAMS', '1')))
_wgrad_streams = {}
_wgrad_rr = {}


# SIDLSG_WGRAD_PRIO=low: the weight-gradient streams are created with the LOWEST HIP stream priority (hipStreamCreateWithPriority; torch
# itself only offers priorities at or above its default stream's), so that the workgroup dispatcher serves the main stream -- the
# backward-data chain, i.e. the critical path -- first and the weight gradients fill what it leaves idle.  A/B knob (profiles/r06_*prio*).
_WGRAD_PRIO = os.environ.get('SIDLSG_WGRAD_PRIO', '')
_hip_rt = None


def _low_priority_stream(device):
    global _hip_rt
    if _hip_rt is None:
        _hip_rt = ctypes.CDLL('libamdhip64.so')          # already in the process (torch's own runtime: same soname)
    least, greatest = ctypes.c_int(0), ctypes.c_int(0)
    if _hip_rt.hipDeviceGetStreamPriorityRange(ctypes.byref(least), ctypes.byref(greatest)) != 0:
        raise RuntimeError('hipDeviceGetStreamPriorityRange failed')
    h = ctypes.c_void_p()
    with torch.cuda.device(device):
        rc = _hip_rt.hipStreamCreateWithPriority(ctypes.byref(h), ctypes.c_uint(1), ctypes.c_int(least.value))      # 1 = hipStreamNonBlocking
    if rc != 0 or not h.value:
        raise RuntimeError(f'hipStreamCreateWithPriority failed with {rc}')
    return torch.cuda.ExternalStream(h.value, device=device)


def _wgrad_stream_list(device):
    key = _dev_key(device)
    if key not in _wgrad_streams:
        lst = [(_low_priority_stream(device) if _WGRAD_PRIO == 'low' else torch.cuda.Stream(device=device)) for _ in range(_WGRAD_NSTREAMS)]
        for st in lst:
            ensure_stream_workspace(st, nbytes=(256 << 20) // _WGRAD_NSTREAMS if _WGRAD_NSTREAMS > 1 else 256 << 20)
        _wgrad_streams[key] = lst
    return _wgrad_streams[key]


def wgrad_stream(device):
    """The stream of the next weight-gradient launch (round robin when several are configured)."""
    lst = _wgrad_stream_list(device)
    if len(lst) > 1 and is_deterministic():
        return lst[0]             # one stream: every gradient is accumulated in one fixed order, across passes too
    key = _dev_key(device)
    i = _wgrad_rr.get(key, 0)
    _wgrad_rr[key] = (i + 1) % len(lst)
    return lst[i]


def wgrad_stream_count():
    """How many streams the weight-gradient launches of a backward pass are spread over.  Two launches on one dW WITHIN a backward pass
    are ordered for any count (_OnWgradStream: the later stream waits for the one that wrote the dW last).  Across passes they are
    ordered through the main stream only: the record of who wrote which dW is dropped at the join that ends a pass, and each launch
    waits for the main stream.  sd_util.hip_generate_steps still refuses the multi-step generator with a count above 1: that
    combination (N uses of every layer in one pass) predates the ordering above and has not been tested with it."""
    return 1 if (not _WGRAD_SIDE or is_deterministic()) else _WGRAD_NSTREAMS


def grad_streams(device):
    """Side streams that may still be writing parameter gradients of `device` (a gradient exchange must wait for them)."""
    return list(_wgrad_streams.get(_dev_key(device), ()))


_wgrad_dw_stream = {}        # several weight-gradient streams only: data_ptr of a dW -> the side stream that wrote it last
wgrad_order_log = None       # a list here records ('launch', dW, stream handle) / ('wait', dW, later handle, earlier handle) (tests)


class _OnWgradStream:
    """with _OnWgradStream(dy, x, dws=(dW, ...)): <wgrad launches> -- inside a torch.autograd.Function.backward only.
    dws: the gradient tensors the launches write.  With one weight-gradient stream two launches on one dW are ordered by the stream.
    With several (SIDLSG_WGRAD_STREAMS > 1) the stream chosen here first waits for the stream that wrote any of `dws` last, so a
    parameter that reaches its weight gradient twice (a shared layer; one use queued and flushed, the other launched directly) is
    accumulated in launch order by construction, whichever streams the round robin hands out."""

    def __init__(self, *tensors, dws=()):
        self.tensors = tensors
        self.dws = dws
        self.on = _WGRAD_SIDE and tensors[0].dtype == BF16

    def __enter__(self):
        if not self.on:
            return self
        dev = self.tensors[0].device
        self.side = wgrad_stream(dev)
        self.side.wait_stream(torch.cuda.current_stream(dev))
        if len(_wgrad_stream_list(dev)) > 1:
            for dw in self.dws:
                p = dw.data_ptr()
                prev = _wgrad_dw_stream.get(p)
                if prev is not None and prev.cuda_stream != self.side.cuda_stream:
                    self.side.wait_stream(prev)
                    if wgrad_order_log is not None:
                        wgrad_order_log.append(('wait', p, self.side.cuda_stream, prev.cuda_stream))
                _wgrad_dw_stream[p] = self.side
                if wgrad_order_log is not None:
                    wgrad_order_log.append(('launch', p, self.side.cuda_stream))
        self.cm = torch.cuda.stream(self.side)
        self.cm.__enter__()
        return self

    def __exit__(self, *exc):
        if not self.on:
            return False
        self.cm.__exit__(*exc)
        for t in self.tensors:
            t.record_stream(self.side)
        # one join per backward pass and device: the mark lives with the pass in the ledger and goes when the pass ends or dies, so a
        # pass that raised cannot leave the next one un-joined and a nested pass does not take the outer one's join away
        dev = self.tensors[0].device
        if _passes.once(('wgrad join', _dev_key(dev))):
            if _wgrad_dw_stream:
                _passes.on_death(_wgrad_dw_stream.clear)     # a pass that dies never joins: its record goes with it
            def join():
                for side in grad_streams(dev):
                    torch.cuda.current_stream(dev).wait_stream(side)
                _wgrad_dw_stream.clear()         # every side stream has been joined: later launches are ordered behind them anyway
            if _passes.current() < 0:            # not inside a backward pass: join right away
                join()
            else:
                torch.autograd.Variable._execution_engine.queue_callback(join)
        return False


# ---- deferred parameter-gradient reductions of the norm backward kernels ---------------------------------------------------
# (csrc/norm.hip "deferred parameter-gradient reductions"): the dgamma / dbeta reductions of a backward pass -- ~80 per trainable
# network and pass, each a tiny launch on the critical stream -- are queued by the library and run as ONE launch per stream when the
# backward pass ends (autograd engine callback), when a gradient-exchange marker fires (_GradReady) or when somebody is about to
# read gradients (flush_deferred(): the fused optimizer and the reducer call it).  The partial-sum workspaces are kept alive here
# until then.  SIDLSG_DEFER_REDUCE=0: one reduction launch per layer as before (A/B, tests).
_DEFER = os.environ.get('SIDLSG_DEFER_REDUCE', '1') != '0'
_defer_streams = {}          # stream handle -> [torch stream, the ledger's queue of (graph-task id, workspace)]


def _defer_begin(device):
    """Before a norm-backward launch that reduces parameter gradients: deferral on for the current stream.
    The library's queue of a stream carries no pass tags, so it holds the reductions of ONE backward pass at a time: what another
    live pass (the outer one of a re-entrant pass) left queued on this stream is launched first -- its partial sums are complete,
    launching them early is harmless -- and a pass that dies can then have exactly its own reductions forgotten."""
    if not _DEFER:
        return None
    st = torch.cuda.current_stream(device)
    h = st.cuda_stream
    key = ('reduce', h)
    if h not in _defer_streams:
        _defer_streams[h] = [st, _passes.queue(key)]
    if _passes.owners(key) - {_passes.current()}:
        _passes.flush(key)
    lib.sidlsg_defer_reductions.raw(h, 1)
    return h


def _defer_end(h, ws):
    """After the launch: keep its partial sums alive; flush at the end of this backward pass (right away outside one)."""
    if h is None:
        return
    lib.sidlsg_defer_reductions.raw(h, 2)        # only the call in between was deferred (direct users of the C ABI never are)
    if _passes.add(('reduce', h), ws) < 0:
        flush_deferred()


def flush_deferred():
    """Launch every queued reduction (one kernel per stream that has any) and order the current stream after them."""
    flush_wgrad_queues()
    _passes.flush()


# ---- grouped dense weight gradients (csrc/wgrad.hip "grouped dense weight gradients") -----------------------------------------------
# The C x C projections of a transformer block (to_out of both attentions, the cross-attention's to_q, proj_in / proj_out) and its
# 77-token k|v projection each need ~56 pixel splits to fill the chip alone.  Their weight gradients are QUEUED here (operands kept
# alive) and launched eight at a time as one grid + one slab reduction (sidlsg_wgrad_group_bf16); whatever is queued is launched when a
# gradient-exchange marker fires, when the backward pass ends, or when somebody is about to read gradients (flush_deferred).
# Only layers that would take the 128 x 128-tile kernel anyway; the wide FF / q|k|v layers keep their 160 x 160-tile launches.
# SIDLSG_WGRAD_GROUP=0: one launch per layer (A/B, tests).
_WG_GROUP = os.environ.get('SIDLSG_WGRAD_GROUP', '1') != '0'
_WG_GROUP160 = os.environ.get('SIDLSG_WGRAD_GROUP160', '1') != '0'      # A/B: the wide layers launch alone (round-5 first version)
_WG_MAX = 8
_WG_MAX160 = 3         # the three wide layers of one transformer block (FF-out, FF-in, q|k|v in backward order): 60 tiles of 160 x 160
_wg_queues = {}          # (stream handle, tile class) -> [torch stream, [jobs], tile class]
_wg_queued_dw = set()    # data_ptr of every dW with a queued job


class _WgJob(ctypes.Structure):
    _fields_ = [('dY', ctypes.c_void_p), ('A', ctypes.c_void_p), ('dW', ctypes.c_void_p), ('dBias', ctypes.c_void_p),
                ('ldy', ctypes.c_int), ('lda', ctypes.c_int), ('M', ctypes.c_int), ('N', ctypes.c_int), ('K', ctypes.c_int),
                ('assign', ctypes.c_int), ('pad', ctypes.c_int * 2)]


def _queue_dense_wgrad(dy, x, dw, dbias, M, N, K, assign, weight=None):
    """True: queued for a grouped launch (the caller must not launch it).
    The jobs of one grouped launch must have DISTINCT dW (include/sidlsg_hip.h): a parameter that reaches its weight gradient twice in
    one backward pass (a shared / re-applied layer; one use queued and another one launched directly) first flushes what is queued
    (the `assign` mark was taken by the earlier one).  The two launches then stay ordered: on the one weight-gradient stream, or --
    several streams -- because the later launch's stream waits for the earlier one's (_OnWgradStream, `dws`).
    A queued job belongs to the backward pass that queued it (the ledger `_passes`): it is launched when its queue is full, at a
    marker, when any live pass ends or before gradients are read; if ITS pass raises it is dropped, never launched, and `weight` gets
    the `assign` mark back that the job had taken (_drop_entries)."""
    if dw.data_ptr() in _wg_queued_dw:
        flush_wgrad_queues()
    if not _WG_GROUP or dy.dtype != BF16 or x.dtype != BF16 or not dy.is_cuda:
        return False
    if (N | K | dy.stride(0) | x.stride(0)) & 7 or (dy.data_ptr() | x.data_ptr()) & 15:
        return False
    # two classes, as in launch_wgrad: the layers of the 160 x 160-tile kernel (q|k|v, FF-in, FF-out: N, K multiples of 160, N != K) are
    # grouped among themselves (sidlsg_wgrad_group160_bf16), everything else on 128 x 128 tiles
    t160 = N % 160 == 0 and K % 160 == 0 and N != K and (M >= 4096 or N * K >= (8 << 20))
    if t160 and not _WG_GROUP160:
        return False
    if _passes.current() < 0:
        return False          # outside a backward pass nobody would flush
    st = torch.cuda.current_stream(dy.device)
    key = ('wgrad', st.cuda_stream, t160)
    q = _wg_queues.setdefault(key[1:], [st, _passes.queue(key), t160])
    _wg_queued_dw.add(dw.data_ptr())
    _passes.add(key, (dy, x, dw, dbias, M, N, K, 1 if assign else 0, weight))
    if len(q[1]) >= (_WG_MAX160 if t160 else _WG_MAX):
        _passes.flush(key)
    return True


def _launch_wgrad_group(st, t160, jobs):
    arr = (_WgJob * len(jobs))()
    for i, (dy, x, dw, dbias, M, N, K, assign, _) in enumerate(jobs):
        arr[i].dY, arr[i].A, arr[i].dW, arr[i].dBias = dy.data_ptr(), x.data_ptr(), dw.data_ptr(), (dbias.data_ptr() if dbias is not None else None)
        arr[i].ldy, arr[i].lda, arr[i].M, arr[i].N, arr[i].K, arr[i].assign = dy.stride(0), x.stride(0), M, N, K, assign
    for j in jobs:                       # launched or not, the jobs have left the queue
        _wg_queued_dw.discard(j[2].data_ptr())
    tensors = [t for j in jobs for t in j[:2]]
    with torch.cuda.stream(st):          # the stream the operands were produced on: the weight-gradient stream waits for IT
        with _OnWgradStream(*tensors, dws=[j[2] for j in jobs]):
            (lib.sidlsg_wgrad_group160_bf16 if t160 else lib.sidlsg_wgrad_group_bf16)(ctypes.addressof(arr), len(jobs), _s())


def flush_wgrad_queues():
    for h, t160 in list(_wg_queues):
        _passes.flush(('wgrad', h, t160))


def _launch_entries(key, entries):
    """Ledger hook: launch what one queue holds.  Every entry is complete work of a LIVE pass (of several, when passes nest)."""
    if key[0] == 'wgrad':
        _launch_wgrad_group(_wg_queues[key[1:]][0], key[2], entries)
    else:
        h = key[1]
        st = _defer_streams[h][0]
        if lib.sidlsg_flush_reductions.raw(h) < 0:
            raise RuntimeError('sidlsg_flush_reductions failed')
        cur = torch.cuda.current_stream(st.device)
        if cur.cuda_stream != h:
            cur.wait_stream(st)


def _drop_entries(key, entries):
    """Ledger hook: the pass that queued `entries` raised.  Launching them into .grad during a later pass -- possibly after an optimizer
    step re-marked the gradients -- would apply stale gradients silently, so they are forgotten: weight-gradient jobs give the `assign`
    mark they took back to their parameter (the next pass must still overwrite what the optimizer left in .grad), and the library
    forgets the dgamma / dbeta reductions queued on the stream (they are this pass's alone, see _defer_begin).  The entries of other
    passes stay.  Gradients the dead pass had already WRITTEN (launches that were not queued, groups that were full) are the caller's
    to zero, as in plain PyTorch."""
    if key[0] == 'wgrad':
        for job in entries:
            _wg_queued_dw.discard(job[2].data_ptr())
            if job[7] and job[8] is not None:
                job[8]._grad_assign = True
    else:
        lib.sidlsg_defer_reductions.raw(key[1], 3)


# The end-of-backward flush: the first entry of a backward pass makes the pass known to the ledger, which queues ONE engine callback
# for it; when it runs -- the pass has ended -- whatever is queued is launched (the entries of every live pass).  A pass is told dead by
# that callback being freed without having run (backward_state.PassLedger); only then, and only for that pass, are entries dropped.
# A nested pass -- a new graph-task id while the outer pass is live -- drops nothing.
_passes = PassLedger(_launch_entries, _drop_entries)


def ensure_stream_workspace(stream, nbytes=256 << 20):
    """Private split-K scratch for a side stream that runs contractions concurrently with the main one."""
    key = stream.cuda_stream
    if key not in _stream_ws:
        ws = torch.empty(nbytes // 4, device=stream.device, dtype=F32)
        lib.sidlsg_set_stream_workspace(key, ws.data_ptr(), ws.numel() * 4)
        _stream_ws[key] = ws
    return _stream_ws[key]


class Fp8Weight:
    """A frozen GEMM / conv weight in the fp8-weight format of include/sidlsg_hip.h: e4m3 bytes [N][K] + one fp32 scale per
    output channel.  Stands where the bf16 compute copy stands in gemm() / conv3x3() (forward only: the backward-data
    operand of a layer stays bf16)."""
    dtype = 'fp8_e4m3'

    def __init__(self, w_bf16):
        w = w_bf16.detach()
        if w.dtype != BF16 or w.ndim != 2 or not w.is_contiguous() or w.shape[1] % 16:
            raise RuntimeError('Fp8Weight: needs a contiguous bf16 [N, K] matrix with K % 16 == 0')
        self.shape = w.shape
        self.q = torch.empty(w.shape, device=w.device, dtype=torch.uint8)
        self.scale = torch.empty(w.shape[0], device=w.device, dtype=F32)
        self.requantize(w)

    def requantize(self, w_bf16):
        lib.sidlsg_quantize_fp8_rows(_p(w_bf16), _p(self.q), _p(self.scale), self.shape[0], self.shape[1], _s())

    def dequantize(self):
        return self.q.view(torch.float8_e4m3fn).float() * self.scale[:, None]


# ---- grouped launches: two networks of identical architecture on one stacked batch ----------------------------------------
class Pair(tuple):
    """(set 0, set 1): the same parameter (forward weight copy, backward-data operand, bias, norm scale / shift) of the two
    networks of a grouped pass.  The first half of the stacked batch is evaluated with set 0, the second half with set 1
    (include/sidlsg_hip.h "grouped launches")."""
    __slots__ = ()

    def __new__(cls, a, b):
        return super().__new__(cls, (a, b))

    @property
    def shape(self):
        return self[0].shape


_dual = None     # while a grouped pass is being recorded: id(tensor of network 0) -> the same tensor of network 1


class dual_networks:
    """`with ops.dual_networks(partner_map): net0.forward_nhwc(stacked inputs)` -- every weight-bearing op issued inside looks
    its parameters' partners up in `partner_map` (HipUNet2DCondition.partner_map(other)) and launches the grouped (`_g2`) entry
    point with both sets; parameter-free ops just see the stacked batch.  The autograd nodes keep the pairs, so the backward
    (data gradients only: both networks are frozen) needs no context."""

    def __init__(self, partner_map):
        self.map = partner_map

    def __enter__(self):
        global _dual
        if _dual is not None:
            raise RuntimeError('grouped passes do not nest')
        _dual = self.map
        return self

    def __exit__(self, *exc):
        global _dual
        _dual = None
        return False


def _pair(t):
    """(t, partner of t) under dual_networks; None stays None."""
    if t is None:
        return None
    try:
        return Pair(t, _dual[id(t)])
    except KeyError:
        raise RuntimeError('grouped pass: a parameter of the first network has no partner in the second one (different '
                           'architectures, fp8 weights, or compute copies re-created after the partner map was built)') from None


def _fp8_pair(w, what):
    """Is this Pair two Fp8Weights (of one shape)?  A pair of one e4m3 and one bf16 copy cannot share a launch."""
    n8 = sum(isinstance(q, Fp8Weight) for q in w)
    if n8 == 1 or (n8 == 2 and w[0].shape != w[1].shape):
        raise RuntimeError(f'{what}: the two weight sets must both be bf16 or both be Fp8Weights, of one shape')
    return n8 == 2


# raw launches
def _weight_args(w):
    """The weight operand of a GEMM / conv launch as the entry points take it: one pointer, (bytes, scales) of an Fp8Weight, or --
    for a Pair of either -- set 0 followed by set 1."""
    if isinstance(w, Pair):
        return _weight_args(w[0]) + _weight_args(w[1])
    if isinstance(w, Fp8Weight):
        return w.q.data_ptr(), w.scale.data_ptr()
    return (w.data_ptr(),)


def _epilogue_args(g2, bias, res, rowvec, res_dim=0, ldres=None):
    """The epilogue operands every GEMM / conv entry point takes after its output: bias (of both sets in a grouped launch), the
    residual and its row stride (`ldres`, else the stride of its dimension `res_dim`), the row vector and its row stride."""
    if res is None:
        ldres = 0
    elif ldres is None:
        ldres = res.stride(res_dim)
    b = (_p(bias),) if not g2 else (None, None) if bias is None else (_p(bias[0]), _p(bias[1]))
    return b + (_p(res), ldres, _p(rowvec), rowvec.stride(0) if rowvec is not None else 0)


def _weight_form(act_dtype, w, what):
    """-> (a Pair?, e4m3 weights?) for the weight operand of a bf16 / fp32 contraction, after the checks gemm() and conv3x3() share."""
    if isinstance(w, Pair):
        f8 = _fp8_pair(w, what)
        if act_dtype != BF16 or (not f8 and (w[0].dtype != BF16 or w[1].dtype != BF16 or w[0].shape != w[1].shape)):
            raise RuntimeError(f'{what}: bf16 activations and two bf16 weight matrices of one shape')
        return True, f8
    if act_dtype == F32 and w.dtype != F32:
        raise RuntimeError('fp32 activations need the fp32 compute copy of the weights')
    f8 = isinstance(w, Fp8Weight)
    if f8 and act_dtype != BF16:
        raise RuntimeError('fp8 weights take bf16 activations')
    return False, f8


def gemm(a, w16, out=None, bias=None, res=None, rowvec=None, rows_per_batch=1, alpha=1.0, out_f32=False, lda=None):
    """C[M,N] = alpha*A[M,K] W[N,K]^T + bias + rowvec[m//rpb] + res.  w16 / bias may be Pairs (grouped launch: rows of the
    first half of A with set 0, of the second half with set 1)."""
    M = a.shape[0]
    K = w16.shape[1]
    N = w16.shape[0]
    lda = a.stride(0) if lda is None else lda
    f32 = a.dtype == F32
    g2, f8 = _weight_form(a.dtype, w16, 'grouped GEMM')
    ensure_workspace(a.device)
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=F32 if (out_f32 or f32) else BF16)
    if f8:
        fn = lib.sidlsg_gemm_fp8w_g2 if g2 else lib.sidlsg_gemm_fp8w
    else:
        fn = lib.sidlsg_gemm_bf16_g2 if g2 else _fn('gemm', a.dtype, '_bf16')
    fn(_p(a), lda, *_weight_args(w16), _p(out), out.stride(0), *_epilogue_args(g2, bias, res, rowvec), rows_per_batch, M, N, K,
       float(alpha), 1 if (out_f32 and not f32) else 0, _s())
    return out


def conv3x3(x, w16, bias=None, res=None, rowvec=None, stride=1, ups=0, out_f32=False, pad=1, silu=False):
    """x: [B,Hs,Ws,Cin] bf16 NHWC; w16: [Cout, 9*Cin]; -> [B,Ho,Wo,Cout].  pad=1: torch's padding=1 on all four sides.
    silu (forward only, pad=1): y = silu(conv + bias + rowvec + res), the SIDLSG_SILU epilogue flag.
    pad='br' (stride 2 only, forward only): zero padding on the bottom and right only -- diffusers Downsample2D(padding=0),
    F.pad(x, (0, 1, 0, 1)) + conv2d(stride=2) (sidlsg_conv3x3_br_bf16); bias is its only epilogue operand."""
    B, Hs, Ws, Cin = x.shape
    if pad == 'br':
        if silu:
            raise RuntimeError("conv3x3(pad='br'): no SiLU epilogue through this wrapper")
        if stride != 2 or ups or res is not None or rowvec is not None or x.dtype != BF16 or isinstance(w16, (Pair, Fp8Weight)) or w16.dtype != BF16:
            raise RuntimeError("conv3x3(pad='br'): stride 2, bf16 activations and weights, no upsampling, residual or row vector")
        if Hs % 2 or Ws % 2:
            raise RuntimeError(f"conv3x3(pad='br'): H and W must be even, got {Hs} x {Ws}")
        Cout = w16.shape[0]
        out = torch.empty((B, Hs // 2, Ws // 2, Cout), device=x.device, dtype=F32 if out_f32 else BF16)
        lib.sidlsg_conv3x3_br_bf16(_p(_chk(x, BF16)), Cin, _p(_chk(w16, BF16)), _p(out), Cout, _p(bias), B, Hs, Ws, Cin, Cout, 1 if out_f32 else 0, _s())
        return out
    if pad != 1:
        raise ValueError(f"conv3x3: pad {pad!r}: expected 1 or 'br'")
    H, W = (2 * Hs, 2 * Ws) if ups else (Hs, Ws)
    Cout = w16.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    f32 = x.dtype == F32
    g2, f8 = _weight_form(x.dtype, w16, 'grouped conv')
    ensure_workspace(x.device)
    out = torch.empty((B, Ho, Wo, Cout), device=x.device, dtype=F32 if (out_f32 or f32) else BF16)
    if f8:
        fn = lib.sidlsg_conv3x3_fp8w_g2 if g2 else lib.sidlsg_conv3x3_fp8w
    else:
        fn = lib.sidlsg_conv3x3_bf16_g2 if g2 else _fn('conv3x3', x.dtype, '_bf16')
    fn(_p(x), Cin, *_weight_args(w16), _p(out), Cout, *_epilogue_args(g2, bias, res, rowvec, ldres=Cout), B, H, W, Cin, Cout, stride, ups,
       1.0, (1 if (out_f32 and not f32) else 0) | (2 if silu else 0), _s())
    return out


def colsum(g2d, rows_per_batch, per_batch=False, total=None, slot=None):
    """g2d: [B*rows_per_batch, N].  total (fp32 [N]) is accumulated in place; returns per-batch sums if asked.
    slot: the (holder, column offset, width) of a split_columns() part -- the per-batch sums are then accumulated straight into the
    part's columns of the holder's shared [B, sum C] gradient buffer (zeroed once per backward pass) and a view of it is returned."""
    R, N = g2d.shape
    B = R // rows_per_batch
    sync_deterministic()
    if per_batch and slot is not None and slot[2] == N:
        holder, off, _ = slot
        buf = holder.buffer(B, g2d.device)
        if buf is not None:
            pb = buf[:, off:off + N]
            _fn('colsum_strided', g2d.dtype)(_p(g2d), g2d.stride(0), pb.data_ptr(), buf.stride(0), _p(total), B, rows_per_batch, N, _s())
            return pb
    pb = torch.zeros((B, N), device=g2d.device, dtype=F32) if per_batch else None
    _fn('colsum', g2d.dtype)(_p(g2d), g2d.stride(0), _p(pb), _p(total), None, B, rows_per_batch, N, _s())
    return pb


def _gradc(t, dtype=BF16):
    """An incoming gradient as the kernels take it: contiguous and of the activation dtype (None stays None)."""
    if t is None:
        return None
    t = t.contiguous()
    return t if t.dtype == dtype else t.to(dtype)


def _conv_dgrad(dy, w16t, x_shape, stride, ups, dtype):
    """Data gradient of conv3x3 (w16t: [Cin, 9*Cout], taps flipped; a Pair in the grouped pass): a stride-2 conv zero-inserts dy
    first, a fused x2 upsample sum-pools the full-resolution gradient down to the input's size."""
    B, Ho, Wo, Cout = dy.shape
    g = dy
    if stride == 2:
        g = torch.empty((B, x_shape[1], x_shape[2], Cout), device=dy.device, dtype=dtype)
        _fn('zero_insert2', dtype)(_p(dy), _p(g), B, Ho, Wo, x_shape[1], x_shape[2], Cout, _s())
    dx = conv3x3(g, w16t)
    if ups:
        full = dx
        dx = torch.empty(x_shape, device=dy.device, dtype=dtype)
        _fn('sumpool2x2', dtype)(_p(full), _p(dx), B, x_shape[1], x_shape[2], x_shape[3], _s())
    return dx


# ------------------------------------------------------------------------------------------------
# One autograd node per weight-bearing op.  A node is in its GROUPED form when its parameters arrive as Pairs (the pass of two
# FROZEN networks over a stacked batch, dual_networks): the backward is then the data gradient only and nothing of the forward
# input is kept alive for a weight gradient -- the Pairs live on ctx (they are not tensors).
# ctx.masters: a weight-bearing node keeps its parameter OBJECTS next to the saved tensors.  The gradient buffer (.grad, `_flat_grad`) and
# the `_grad_assign` mark hang on the object, and ctx.saved_tensors does not always give it back: under saved-tensor hooks -- the
# recomputation of torch.utils.checkpoint(use_reentrant=False) -- a saved parameter returns as a detached alias that has neither.  The
# saved tensors are still unpacked (values, and autograd's check that nothing was modified in place); only the identity comes from ctx.
class _Linear(torch.autograd.Function):
    """y = x W^T + b (+ res) (+ rowvec broadcast over rows_per_batch rows).  x: [M,K] bf16.  Grouped: bias / w16 / w16t are Pairs and
    weight is None."""

    @staticmethod
    def forward(ctx, x, weight, bias, w16, w16t, res, rowvec, rows_per_batch, out_f32):
        ctx.g2 = isinstance(w16, Pair)
        _chk(x, BF16 if ctx.g2 else ACT)
        y = gemm(x, w16, bias=bias, res=res, rowvec=rowvec, rows_per_batch=rows_per_batch, out_f32=out_f32)
        if ctx.g2:
            ctx.w16t = w16t
        else:
            ctx.save_for_backward(x, weight, bias, w16t)
            ctx.masters = (weight, bias)
        ctx.dtype = x.dtype
        ctx.rpb = rows_per_batch
        ctx.has_res = res is not None
        ctx.has_rv = rowvec is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _gradc(dy, ctx.dtype)
        need_rv = ctx.has_rv and ctx.needs_input_grad[6]
        dres = dy if (ctx.has_res and ctx.needs_input_grad[5]) else None
        if ctx.g2:
            dx = gemm(dy, ctx.w16t) if ctx.needs_input_grad[0] else None
            drv = colsum(dy, ctx.rpb, per_batch=True) if need_rv else None
            return dx, None, None, None, None, dres, drv, None, None
        x, _, _, w16t = ctx.saved_tensors
        weight, bias = ctx.masters
        dx = gemm(dy, w16t) if ctx.needs_input_grad[0] else None
        need_b = _wants_grad(bias)
        # bias gradient comes out of the bf16 wgrad kernel (the fp32 family computes it with a column sum)
        fused_b = need_b and not need_rv and _wants_grad(weight) and x.dtype == BF16
        if _wants_grad(weight):
            M, K = x.shape
            assign = _take_assign(weight, x.dtype)
            if not _queue_dense_wgrad(dy, x, weight.grad, bias.grad if fused_b else None, M, weight.shape[0], K, assign, weight):
                wg = _fn('wgrad_assign', x.dtype, '_bf16') if assign else _fn('wgrad', x.dtype, '_bf16')
                with _OnWgradStream(dy, x, dws=(weight.grad,)):
                    wg(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(weight.grad), _p(bias.grad) if fused_b else None, M, weight.shape[0], K, _s())
        drv = None
        if need_rv:
            drv = colsum(dy, ctx.rpb, per_batch=True, total=bias.grad if need_b else None)
        elif need_b and not fused_b:
            colsum(dy, dy.shape[0], total=bias.grad)
        return dx, None, None, None, None, dres, drv, None, None


def _frozen(*params):
    for p in params:
        for q in (p if isinstance(p, Pair) else (p,)):
            if q is not None and q.requires_grad:
                raise RuntimeError('a grouped pass evaluates FROZEN networks: call requires_grad_(False) on both first')


def linear(x, weight, bias, w16, w16t, res=None, rowvec=None, rows_per_batch=1, out_f32=False):
    if _dual is not None:
        wp, bp = _pair(weight), _pair(bias)
        _frozen(wp, bp)
        return _Linear.apply(x, None, bp, _pair(w16), _pair(w16t), res, rowvec, rows_per_batch, out_f32)
    if isinstance(w16, Fp8Weight):
        _mx8_no_weight_grads(weight, None)
    return _Linear.apply(x, weight, bias, w16, w16t, res, rowvec, rows_per_batch, out_f32)


class _Conv3x3(torch.autograd.Function):
    """NHWC 3x3 conv, pad 1, stride 1|2, optional fused nearest-x2 upsample of the input.  Grouped: bias / w16 / w16t are Pairs and
    weight is None."""

    @staticmethod
    def forward(ctx, x, weight, bias, w16, w16t, res, rowvec, stride, ups, out_f32, bias_p):
        ctx.g2 = isinstance(w16, Pair)
        _chk(x, BF16 if ctx.g2 else ACT)
        y = conv3x3(x, w16, bias=bias_p if bias_p is not None else bias, res=res, rowvec=rowvec, stride=stride, ups=ups,
                    out_f32=out_f32)
        if ctx.g2:
            ctx.w16t = w16t
        else:
            ctx.save_for_backward(x, weight, bias, w16t)
            ctx.masters = (weight, bias)
        ctx.cfg = (stride, ups, res is not None, rowvec is not None, x.shape, x.dtype)
        ctx.rv_slot = getattr(rowvec, '_col_slot', None)
        return y

    @staticmethod
    def backward(ctx, dy):
        stride, ups, has_res, has_rv, xs, dtype = ctx.cfg
        dy = _gradc(dy, dtype)
        B, Ho, Wo, Cout = dy.shape
        dy2 = dy.view(B * Ho * Wo, Cout)
        need_rv = has_rv and ctx.needs_input_grad[6]
        dres = dy if (has_res and ctx.needs_input_grad[5]) else None
        if ctx.g2:
            dx = _conv_dgrad(dy, ctx.w16t, xs, stride, ups, dtype) if ctx.needs_input_grad[0] else None
            drv = colsum(dy2, Ho * Wo, per_batch=True, slot=ctx.rv_slot) if need_rv else None
            return dx, None, None, None, None, dres, drv, None, None, None, None
        x, _, _, w16t = ctx.saved_tensors
        weight, bias = ctx.masters
        Cin = xs[3]
        dx = _conv_dgrad(dy, w16t, xs, stride, ups, dtype) if ctx.needs_input_grad[0] else None
        co_w, ci_w = weight.shape[0], weight.shape[1]     # logical (unpadded) sizes of the master
        padded = (co_w != Cout) or (ci_w != Cin)           # conv_in (Cin 4->8) / conv_out (Cout 4->8)
        need_b = _wants_grad(bias)
        # bias gradient from the (bf16) wgrad kernel
        fused_b = need_b and not need_rv and not padded and _wants_grad(weight) and x.dtype == BF16
        if _wants_grad(weight):
            H, W = (2 * xs[1], 2 * xs[2]) if ups else (xs[1], xs[2])
            wgrad = _fn('conv3x3_wgrad', x.dtype, '_bf16')
            if not padded and _take_assign(weight, x.dtype):
                wgrad = lib.sidlsg_conv3x3_wgrad_assign_bf16
            if not padded:
                with _OnWgradStream(dy, x, dws=(weight.grad,)):
                    wgrad(_p(dy), Cout, _p(x), Cin, _p(weight.grad), _p(bias.grad) if fused_b else None,
                          B, H, W, Cin, Cout, stride, ups, _s())
            else:
                tmp = torch.zeros((Cout, 9, Cin), device=dy.device, dtype=F32)
                wgrad(_p(dy), Cout, _p(x), Cin, _p(tmp), None, B, H, W, Cin, Cout, stride, ups, _s())
                weight.grad.permute(0, 2, 3, 1).reshape(co_w, 9, ci_w).add_(tmp[:co_w, :, :ci_w])
        drv = None
        btot = None
        if need_b and not fused_b:
            btot = bias.grad if co_w == Cout else torch.zeros(Cout, device=dy.device, dtype=F32)
        if need_rv:
            drv = colsum(dy2, Ho * Wo, per_batch=True, total=btot, slot=ctx.rv_slot)
        elif need_b and not fused_b:
            colsum(dy2, dy2.shape[0], total=btot)
        if need_b and not fused_b and co_w != Cout:
            bias.grad.add_(btot[:co_w])
        return dx, None, None, None, None, dres, drv, None, None, None, None


def conv3x3_op(x, weight, bias, w16, w16t, res=None, rowvec=None, stride=1, ups=0, out_f32=False, bias_p=None):
    if _dual is not None:
        wp, bp = _pair(weight), _pair(bias)
        _frozen(wp, bp)
        bq = _pair(bias_p) if bias_p is not None else bp        # (conv_out: the zero-padded bias of the padded output channels)
        return _Conv3x3.apply(x, None, bq, _pair(w16), _pair(w16t), res, rowvec, stride, ups, out_f32, None)
    if isinstance(w16, Fp8Weight):
        _mx8_no_weight_grads(weight, None)
    return _Conv3x3.apply(x, weight, bias, w16, w16t, res, rowvec, stride, ups, out_f32, bias_p)


# ---- norm launches: parameters are tensors, or Pairs (samples / token rows of the first half of the batch with set 0, the others set 1) ----
def _groupnorm_fwd(x, gamma, beta, groups, eps, silu, out_e4m3=False):
    """GroupNorm (+ SiLU) of x [B, ..., C] -> (y, stats, ws floats); out_e4m3: y as e4m3 bytes (uint8; bf16 x only)."""
    g2 = isinstance(gamma, Pair)
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    n = lib.sidlsg_groupnorm_ws_floats.raw(B, HW, C, groups)
    if n < 0 or (g2 and B % 2):
        raise RuntimeError(f'{"grouped " if g2 else ""}groupnorm: unsupported shape B={B} HW={HW} C={C} G={groups}')
    ws = torch.empty(n, device=x.device, dtype=F32)
    stats = torch.empty((B, groups, 2), device=x.device, dtype=F32)
    y = torch.empty(x.shape, device=x.device, dtype=torch.uint8) if out_e4m3 else torch.empty_like(x)
    if g2:
        fn = lib.sidlsg_groupnorm_fwd_fp8_g2 if out_e4m3 else lib.sidlsg_groupnorm_fwd_g2
        params = (_p(gamma[0]), _p(beta[0]), _p(gamma[1]), _p(beta[1]))
    else:
        fn = lib.sidlsg_groupnorm_fwd_fp8 if out_e4m3 else _fn('groupnorm_fwd', x.dtype)
        params = (_p(gamma), _p(beta))
    fn(_p(x), *params, _p(y), _p(stats), _p(ws), B, HW, C, groups, float(eps), int(silu), _s())
    return y, stats, n


def _groupnorm_bwd(x, dy, stats, gamma, beta, dkeep, cfg, param_grads=False):
    """-> dx (+ dkeep, summed inside the kernel).  cfg: (groups, silu, ws floats) of the forward.  param_grads: also reduce dgamma /
    dbeta into the parameters' .grad where they want one (the single trainable form; a Pair is frozen)."""
    groups, silu, n = cfg
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    ws = torch.empty(n, device=x.device, dtype=F32)
    dx = torch.empty_like(x)
    if isinstance(gamma, Pair):
        lib.sidlsg_groupnorm_bwd_g2(_p(x), _p(dy), _p(stats), _p(gamma[0]), _p(beta[0]), _p(gamma[1]), _p(beta[1]), _p(dkeep), _p(dx), _p(ws),
                                    B, HW, C, groups, silu, _s())
        return dx
    pg = param_grads and _wants_grad(gamma) and _wants_grad(beta)
    h = _defer_begin(x.device) if pg else None
    _fn('groupnorm_bwd', x.dtype)(_p(x), _p(dy), _p(stats), _p(gamma), _p(beta), _p(dkeep), _p(dx), _p(gamma.grad) if pg else None,
                                  _p(beta.grad) if pg else None, _p(ws), B, HW, C, groups, silu, _s())
    _defer_end(h, ws)
    return dx


def _row(t, r):
    """Address of row r of a contiguous [..., C] tensor seen as [rows, C] (None stays None)."""
    return None if t is None else t.view(-1, t.shape[-1])[r:].data_ptr()


def _layernorm_fwd(x, gamma, beta, eps, out_e4m3=False):
    """LayerNorm of x [..., C] -> (y, stats, grouped); out_e4m3: y as e4m3 bytes (uint8; bf16 x only).  grouped: the two-set kernel
    ran.  Halves whose row count it cannot align its per-wave row ranges with (tiny test networks) run as two ordinary launches on
    the half views."""
    C = x.shape[-1]
    rows = x.numel() // C
    g2 = isinstance(gamma, Pair)
    if g2 and rows % 2:
        raise RuntimeError('grouped layernorm: odd row count')
    y = torch.empty(x.shape, device=x.device, dtype=torch.uint8) if out_e4m3 else torch.empty_like(x)
    stats = torch.empty((rows, 2), device=x.device, dtype=F32)
    half = rows // 2
    if g2 and half % 16 == 0:
        (lib.sidlsg_layernorm_fwd_fp8_g2 if out_e4m3 else lib.sidlsg_layernorm_fwd_g2)(
            _p(x), _p(gamma[0]), _p(beta[0]), _p(gamma[1]), _p(beta[1]), _p(y), _p(stats), rows, C, float(eps), _s())
        return y, stats, True
    single = lib.sidlsg_layernorm_fwd_fp8 if out_e4m3 else _fn('layernorm_fwd', x.dtype)
    if not g2:
        single(_p(x), _p(gamma), _p(beta), _p(y), _p(stats), rows, C, float(eps), _s())
    else:
        for h in (0, 1):
            single(_row(x, h * half), _p(gamma[h]), _p(beta[h]), _row(y, h * half), _row(stats, h * half), half, C, float(eps), _s())
    return y, stats, False


def _layernorm_bwd(x, dy, stats, gamma, beta, dkeep, grouped, param_grads=False):
    """-> dx (+ dkeep).  grouped: what _layernorm_fwd returned; param_grads: as in _groupnorm_bwd."""
    C = x.shape[-1]
    rows = x.numel() // C
    dx = torch.empty_like(x)
    if grouped:
        lib.sidlsg_layernorm_bwd_g2(_p(x), _p(dy), _p(stats), _p(gamma[0]), _p(gamma[1]), _p(dkeep), _p(dx), rows, C, _s())
        return dx
    single = _fn('layernorm_bwd', x.dtype)
    if not isinstance(gamma, Pair):
        pg = param_grads and _wants_grad(gamma) and _wants_grad(beta)
        ws = torch.empty(lib.sidlsg_layernorm_bwd_nblocks.raw(rows) * C * 2, device=x.device, dtype=F32) if pg else None
        h = _defer_begin(x.device) if pg else None
        single(_p(x), _p(dy), _p(stats), _p(gamma), _p(dkeep), _p(dx), _p(gamma.grad) if pg else None, _p(beta.grad) if pg else None,
               _p(ws), rows, C, _s())
        _defer_end(h, ws)
    else:
        half = rows // 2
        for h in (0, 1):
            r = h * half
            single(_row(x, r), _row(dy, r), _row(stats, r), _p(gamma[h]), _row(dkeep, r), _row(dx, r), None, None, None, half, C, _s())
    return dx


def groupnorm_fp8_g2(x, gamma, beta, groups, eps, silu):
    """Grouped GroupNorm (+ SiLU) with an e4m3 output: x [B, ..., C] bf16 (B even), gamma / beta (set 0, set 1) -> (y8, stats, ws floats)."""
    return _groupnorm_fwd(x, Pair(*gamma), Pair(*beta), groups, eps, silu, out_e4m3=True)


def layernorm_fp8_g2(x, gamma, beta, eps):
    """Grouped LayerNorm with an e4m3 output: x [..., C] bf16 (even row count), gamma / beta (set 0, set 1) -> (y8, stats, grouped)."""
    return _layernorm_fwd(x, Pair(*gamma), Pair(*beta), eps, out_e4m3=True)


def _keep(ctx, x, stats, *params):
    """What a norm node keeps for its backward: x and stats as saved tensors, and its parameters -- saved tensors too in the single
    form (and as `ctx.masters`, see there), Pairs on ctx in the grouped one."""
    if isinstance(params[0], Pair):
        ctx.save_for_backward(x, stats)
        ctx.params = params
    else:
        ctx.save_for_backward(x, stats, *params)
        ctx.params, ctx.masters = None, params


def _kept(ctx):
    """-> x, stats, parameters as _keep() got them."""
    x, stats, *_ = ctx.saved_tensors
    return x, stats, ctx.params or ctx.masters


class _GroupNorm(torch.autograd.Function):
    """fork=True: returns (y, x_keep) where x_keep aliases x and must be what the block's OTHER branch (residual /
    shortcut) consumes.  The gradient of that branch then arrives here as dkeep and is summed inside the norm-backward
    kernel instead of by a separate autograd accumulation kernel (~1.5 % of the step)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, silu, fork):
        _chk(x, BF16 if isinstance(gamma, Pair) else ACT)
        y, stats, n = _groupnorm_fwd(x, gamma, beta, groups, eps, silu)
        _keep(ctx, x, stats, gamma, beta)
        ctx.cfg = (groups, int(silu), n)
        if fork:
            return y, x.view(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy, dkeep=None):
        if dy is None:                       # only the pass-through output was used
            return dkeep, None, None, None, None, None, None
        x, stats, (gamma, beta) = _kept(ctx)
        dx = _groupnorm_bwd(x, _gradc(dy, x.dtype), stats, gamma, beta, _gradc(dkeep, x.dtype), ctx.cfg, param_grads=True)
        return dx, None, None, None, None, None, None


def group_norm(x, gamma, beta, groups, eps, silu, fork=False):
    if _dual is not None:
        gamma, beta = _pair(gamma), _pair(beta)
        _frozen(gamma, beta)
    return _GroupNorm.apply(x, gamma, beta, groups, eps, silu, fork)


class _LayerNorm(torch.autograd.Function):
    """fork=True: see _GroupNorm."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, fork):
        _chk(x, BF16 if isinstance(gamma, Pair) else ACT)
        y, stats, ctx.grouped = _layernorm_fwd(x, gamma, beta, eps)
        _keep(ctx, x, stats, gamma, beta)
        if fork:
            return y, x.view(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy, dkeep=None):
        if dy is None:
            return dkeep, None, None, None, None
        x, stats, (gamma, beta) = _kept(ctx)
        dx = _layernorm_bwd(x, _gradc(dy, x.dtype), stats, gamma, beta, _gradc(dkeep, x.dtype), ctx.grouped, param_grads=True)
        return dx, None, None, None, None


def layer_norm(x, gamma, beta, eps=1e-5, fork=False):
    if _dual is not None:
        gamma, beta = _pair(gamma), _pair(beta)
        _frozen(gamma, beta)
    return _LayerNorm.apply(x, gamma, beta, eps, fork)


def gemm_mx8(a8, w8, out=None, bias=None, res=None, out_f32=False):
    """C[M,N] = wscale[n] * A8[M,K] W8[N,K]^T + bias + res with BOTH operands e4m3 (sidlsg_gemm_mx8: MX MFMA).
    a8: uint8 [M,K] e4m3 bytes at unit scale; w8: Fp8Weight with N % 160 == 0.  Inside dual_networks (or with w8 / bias given as
    Pairs) the grouped launch: rows of the first half of a8 with set 0, of the second half with set 1."""
    if _dual is not None and not isinstance(w8, Pair):
        w8, bias = _pair(w8), _pair(bias)
    g2 = isinstance(w8, Pair)
    if a8.dtype != torch.uint8 or not (_fp8_pair(w8, 'gemm_mx8') if g2 else isinstance(w8, Fp8Weight)):
        raise RuntimeError('gemm_mx8: e4m3 activations (uint8) and an Fp8Weight')
    M, K = a8.shape
    N = w8.shape[0]
    ensure_workspace(a8.device)
    if out is None:
        out = torch.empty((M, N), device=a8.device, dtype=F32 if out_f32 else BF16)
    (lib.sidlsg_gemm_mx8_g2 if g2 else lib.sidlsg_gemm_mx8)(
        _p(a8), a8.stride(0), *_weight_args(w8), _p(out), out.stride(0), *_epilogue_args(g2, bias, res, None), 1, M, N, K, 1.0,
        1 if out_f32 else 0, _s())
    return out


def conv3x3_mx8(x8, w8, bias=None, res=None, rowvec=None, out_f32=False):
    """3x3 conv, pad 1, stride 1, on an e4m3 NHWC image x8 [B,H,W,Cin] (uint8) with an Fp8Weight [Cout, 9*Cin] (Cout % 160 == 0).
    Inside dual_networks (or with w8 / bias given as Pairs) the grouped launch: samples of the first half with set 0, the others set 1."""
    if _dual is not None and not isinstance(w8, Pair):
        w8, bias = _pair(w8), _pair(bias)
    g2 = isinstance(w8, Pair)
    if x8.dtype != torch.uint8 or not (_fp8_pair(w8, 'conv3x3_mx8') if g2 else isinstance(w8, Fp8Weight)):
        raise RuntimeError('conv3x3_mx8: e4m3 activations (uint8) and an Fp8Weight')
    B, H, W, Cin = x8.shape
    Cout = w8.shape[0]
    ensure_workspace(x8.device)
    out = torch.empty((B, H, W, Cout), device=x8.device, dtype=F32 if out_f32 else BF16)
    (lib.sidlsg_conv3x3_mx8_g2 if g2 else lib.sidlsg_conv3x3_mx8)(
        _p(x8), x8.stride(2), *_weight_args(w8), _p(out), Cout, *_epilogue_args(g2, bias, res, rowvec, res_dim=2), B, H, W, Cin, Cout, 1.0,
        1 if out_f32 else 0, _s())
    return out


def cast_fp8(x):
    """bf16 [.., K] -> e4m3 bytes (uint8, same shape): clamp to +-448, round to nearest even, unit scale."""
    _chk(x, BF16)
    y = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    lib.sidlsg_cast_fp8(_p(x), _p(y), x.numel(), _s())
    return y


def mx8_ok(w):
    """Can this forward weight take e4m3 activations through sidlsg_gemm_mx8?"""
    return isinstance(w, Fp8Weight) and w.shape[0] % 160 == 0 and w.shape[1] % 16 == 0


class _NormLinear(torch.autograd.Function):
    """FROZEN networks with e4m3 weights: y = Linear(Norm(x)) as ONE autograd node -- the GroupNorm / LayerNorm kernel writes
    its output as e4m3 bytes (half the bytes of the bf16 output it replaces), the contraction runs on the MX-fp8 MFMA
    (gemm_mx8).  One node because the e4m3 intermediate is an integer tensor autograd cannot carry.  Backward (the data
    gradient the generator's update needs through the frozen networks): dnorm_out = dy W through the bf16 backward-data
    operand, then the ordinary norm backward on the saved input.  fork: as in _GroupNorm / _LayerNorm.  Grouped (two frozen e4m3
    networks): gamma / beta / w8 / bias / w16t are Pairs, every launch is the two-set one."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, groups, silu, fork, w8, bias, w16t, weight):
        _chk(x, BF16)
        if groups:
            y8, stats, n = _groupnorm_fwd(x, gamma, beta, groups, eps, silu, out_e4m3=True)
            ctx.cfg = (groups, int(silu), n)
        else:
            y8, stats, ctx.grouped = _layernorm_fwd(x, gamma, beta, eps, out_e4m3=True)
            ctx.cfg = None
        y = gemm_mx8(y8.view(-1, x.shape[-1]), w8, bias=bias)
        _keep(ctx, x, stats, gamma, beta, w16t)
        if fork:
            return y, x.view(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy, dkeep=None):
        none = (None,) * 10
        if dy is None:
            return (dkeep,) + none
        x, stats, (gamma, beta, w16t) = _kept(ctx)
        dn = gemm(_gradc(dy), w16t)                                # gradient at the norm's output, [M, C]
        dkeep = _gradc(dkeep)
        if ctx.cfg is not None:
            dx = _groupnorm_bwd(x, dn, stats, gamma, beta, dkeep, ctx.cfg)
        else:
            dx = _layernorm_bwd(x, dn, stats, gamma, beta, dkeep, ctx.grouped)
        return (dx,) + none


class _NormConv(torch.autograd.Function):
    """FROZEN networks: y = conv3x3(SiLU(GroupNorm(x))) + bias + rowvec (+ res) as one autograd node with the e4m3 image in
    between (see _NormLinear).  Backward: data gradient of the conv through the bf16 backward-data operand (flipped taps),
    then the GroupNorm + SiLU backward on the saved input; res receives dy, rowvec its per-sample column sums.  Grouped: as
    _NormLinear."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, groups, fork, w8, bias, w16t, weight, res, rowvec):
        _chk(x, BF16)
        y8, stats, n = _groupnorm_fwd(x, gamma, beta, groups, eps, 1, out_e4m3=True)
        y = conv3x3_mx8(y8, w8, bias=bias, res=res, rowvec=rowvec)
        _keep(ctx, x, stats, gamma, beta, w16t)
        ctx.cfg = (groups, 1, n)
        ctx.has_res, ctx.has_rv = res is not None, rowvec is not None
        ctx.rv_slot = getattr(rowvec, '_col_slot', None)
        if fork:
            return y, x.view(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy, dkeep=None):
        if dy is None:
            return (dkeep,) + (None,) * 11
        x, stats, (gamma, beta, w16t) = _kept(ctx)
        dy = _gradc(dy)
        dn = _conv_dgrad(dy, w16t, x.shape, 1, 0, BF16)           # gradient at the conv's input, [B,H,W,C]
        dx = _groupnorm_bwd(x, dn, stats, gamma, beta, _gradc(dkeep), ctx.cfg)
        dres = dy if (ctx.has_res and ctx.needs_input_grad[10]) else None
        drv = None
        if ctx.has_rv and ctx.needs_input_grad[11]:
            B, H, W, Cout = dy.shape
            drv = colsum(dy.view(B * H * W, Cout), H * W, per_batch=True, slot=ctx.rv_slot)
        return (dx,) + (None,) * 9 + (dres, drv)


def _mx8_no_weight_grads(weight, gamma):
    """The e4m3 forward has no weight-gradient backward: fine under no_grad and for frozen parameters, an error otherwise."""
    if torch.is_grad_enabled() and ((weight is not None and weight.requires_grad) or (gamma is not None and gamma.requires_grad)):
        raise RuntimeError('the MX-fp8 path is for passes without weight gradients (frozen network, or torch.no_grad())')


def _mx8_params(weight, gamma, beta, w8, bias, w16t):
    """The parameters of an e4m3 node as it takes them: as they are (after the frozen check) or, inside dual_networks, as Pairs."""
    if _dual is None:
        _mx8_no_weight_grads(weight, gamma)
        return weight, gamma, beta, w8, bias, w16t
    wp, gp, bp, cb = _pair(weight), _pair(gamma), _pair(beta), _pair(bias)
    _frozen(wp, gp, bp, cb)
    return None, gp, bp, _pair(w8), cb, _pair(w16t)


def norm_conv_mx8(x, gamma, beta, eps, groups, w8, bias, w16t, weight, res=None, rowvec=None, fork=False):
    """conv3x3(SiLU(GroupNorm(x))) for a frozen network, e4m3 in between."""
    weight, gamma, beta, w8, bias, w16t = _mx8_params(weight, gamma, beta, w8, bias, w16t)
    return _NormConv.apply(x, gamma, beta, eps, groups, fork, w8, bias, w16t, weight, res, rowvec)


def norm_linear_mx8(x, gamma, beta, eps, w8, bias, w16t, weight, groups=0, silu=False, fork=False):
    """Linear(GroupNorm(x)) (groups > 0) or Linear(LayerNorm(x)) (groups = 0) for a frozen network, e4m3 in between."""
    weight, gamma, beta, w8, bias, w16t = _mx8_params(weight, gamma, beta, w8, bias, w16t)
    return _NormLinear.apply(x, gamma, beta, eps, groups, silu, fork, w8, bias, w16t, weight)


_ATTN_ALWAYS_KV = os.environ.get('SIDLSG_ATTN_SKIP_KV', '1') == '0'      # A/B switch: compute dK / dV even when nobody wants them


ATTN_HEAD_WIDTHS = (16, 32, 48, 64, 80, 96, 128, 160)      # the head widths csrc/attention.hip and csrc/fp32.hip are tiled for


def _attn_head_width(D, dtype):
    """The widths sidlsg_attn_fwd / _bwd (and _ps, _f32) admit, include/sidlsg_hip.h: said here in words, not as code -22."""
    step = 4 if dtype == F32 else 8
    if D <= 0 or D % step or (D + 15) // 16 * 16 not in ATTN_HEAD_WIDTHS:
        raise RuntimeError(f'attention: head width {D} is not admitted: it must be a multiple of {step} whose round-up to a multiple of 16 '
                           f'is one of {", ".join(map(str, ATTN_HEAD_WIDTHS))} (there are no kernels for 112 and 144)')


class _Attention(torch.autograd.Function):
    """q: [B,Nq,*] view with heads*D channels starting at column qoff of a row of width ldq; same for k, v."""

    @staticmethod
    def forward(ctx, qbuf, kvbuf, heads, D, qoff, koff, voff, prescaled=False):
        _chk(qbuf, ACT)
        _chk(kvbuf, qbuf.dtype)
        # prescaled: the queries arrive multiplied by D^-1/2 log2(e) (folded into the projection's forward weight copy,
        # HipUNet2DCondition._build_prescale_plan) -> the `_ps` entry points; bf16 only
        sfx = '_ps' if (prescaled and qbuf.dtype == BF16) else ''
        if prescaled and not sfx:
            raise RuntimeError('pre-scaled queries exist in the bf16 compute mode only')
        _attn_head_width(D, qbuf.dtype)
        B, Nq, ldq = qbuf.shape
        Nk, ldk = kvbuf.shape[1], kvbuf.shape[2]
        C = heads * D
        o = torch.empty((B, Nq, C), device=qbuf.device, dtype=qbuf.dtype)
        lse = torch.empty((B, heads, Nq), device=qbuf.device, dtype=F32)
        es = qbuf.element_size()
        _fn('attn_fwd' + sfx, qbuf.dtype)(qbuf.data_ptr() + qoff * es, kvbuf.data_ptr() + koff * es, kvbuf.data_ptr() + voff * es, _p(o), _p(lse),
                                    B, heads, Nq, Nk, D, ldq, ldk, ldk, C, Nq * ldq, Nk * ldk, Nk * ldk, Nq * C, _s())
        ctx.save_for_backward(qbuf, kvbuf, o, lse)
        ctx.cfg = (heads, D, qoff, koff, voff, sfx)
        return o

    @staticmethod
    def backward(ctx, do):
        qbuf, kvbuf, o, lse = ctx.saved_tensors
        heads, D, qoff, koff, voff, sfx = ctx.cfg
        B, Nq, ldq = qbuf.shape
        Nk, ldk = kvbuf.shape[1], kvbuf.shape[2]
        C = heads * D
        do = do.contiguous()
        if do.dtype != qbuf.dtype:
            do = do.to(qbuf.dtype)
        same = qbuf.data_ptr() == kvbuf.data_ptr()
        # cross-attention whose keys / values nobody differentiates (frozen k|v projection of the text states): dQ only
        need_kv = same or ctx.needs_input_grad[1] or _ATTN_ALWAYS_KV
        dq = torch.empty_like(qbuf)
        dkv = dq if same else (torch.empty_like(kvbuf) if need_kv else None)
        delta = torch.empty((B, heads, Nq), device=qbuf.device, dtype=F32)
        es = qbuf.element_size()
        _fn('attn_bwd' + sfx, qbuf.dtype)(qbuf.data_ptr() + qoff * es, kvbuf.data_ptr() + koff * es, kvbuf.data_ptr() + voff * es, _p(o), _p(do),
                            _p(lse), dq.data_ptr() + qoff * es, dkv.data_ptr() + koff * es if need_kv else None,
                            dkv.data_ptr() + voff * es if need_kv else None, _p(delta),
                            B, heads, Nq, Nk, D, ldq, ldk, ldk, C, Nq * ldq, Nk * ldk, Nk * ldk, Nq * C, _s())
        return dq, (None if same else dkv), None, None, None, None, None, None


WIDE_HEAD = 512      # the one head width of sidlsg_attn_fwd_wide


def wide_attention(q, k, v):
    """softmax(q k^T / sqrt(D)) v for ONE head of width D = 512 (the VAE mid-block attention; sidlsg_attn_fwd_wide): q, k, v
    [B, N, 512] bf16, contiguous or column slices of a wider [B, N, ld] buffer (a fused q|k|v projection); N a multiple of 16.
    Forward only; -> [B, N, 512] bf16."""
    for t in (q, k, v):
        if not t.is_cuda:
            raise RuntimeError('sid_lsg_amd ops need CUDA(HIP) tensors: there is no CPU fallback')
        if t.dtype != BF16 or t.dim() != 3 or t.shape != q.shape or t.stride(2) != 1:
            raise RuntimeError(f'wide_attention: expected three bf16 [B, N, D] tensors of one shape with unit channel stride, got {tuple(t.shape)} {t.dtype}')
    B, N, D = q.shape
    o = torch.empty((B, N, D), device=q.device, dtype=BF16)
    lib.sidlsg_attn_fwd_wide(_p(q), _p(k), _p(v), _p(o), B, N, D, q.stride(1), k.stride(1), v.stride(1), D, q.stride(0), k.stride(0), v.stride(0),
                             N * D, _s())
    return o


def self_attention(qkv, heads, prescaled=False):
    """qkv: [B,N,3C] (fused projection output) -> [B,N,C]"""
    C = qkv.shape[2] // 3
    return _Attention.apply(qkv, qkv, heads, C // heads, 0, C, 2 * C, prescaled)


def cross_attention(q, kv, heads, prescaled=False):
    """q: [B,N,C]; kv: [B,L,2C] (fused k|v projection of the text states) -> [B,N,C]"""
    C = q.shape[2]
    return _Attention.apply(q, kv, heads, C // heads, 0, 0, C, prescaled)


CROSS2_MAX_KEYS = 128         # sidlsg_attn_cross2_fwd: text keys of one (batch, head), staged in one workgroup's LDS
CROSS2_MAX_KEYS2 = 32         # ... and image keys
CROSS2_LDS_BYTES = 160 * 1024


def cross_attention2(q, kv, k2v2, heads, s, prescaled=False):
    """softmax(q k^T / sqrt(D)) v + s * softmax(q k2^T / sqrt(D)) v2 per head in ONE launch (sidlsg_attn_cross2_fwd, csrc/ip_attn.hip):
    the decoupled cross-attention of an image-prompt adapter.  q: [B, N, C]; kv: [B, L, 2C] (the fused k|v projection of the text
    states); k2v2: [B, T, 2C], the adapter's k|v for this layer -- contiguous or a column slice of a wider per-batch buffer (unit
    channel stride; its row and batch strides are passed on).  1 <= L <= 128, 1 <= T <= 32; C / heads a multiple of 8 (fp32: 4) up to
    160.  Forward only: refuses enabled autograd on an input that requires grad.  -> [B, N, C]."""
    _chk(q, ACT)
    _chk(kv, q.dtype)
    if not k2v2.is_cuda or k2v2.dtype != q.dtype:
        raise RuntimeError(f'cross_attention2: the image keys / values must be {q.dtype} CUDA(HIP) tensors, got {k2v2.dtype} on {k2v2.device}')
    if torch.is_grad_enabled() and (q.requires_grad or kv.requires_grad or k2v2.requires_grad):
        raise RuntimeError('cross_attention2 is forward only (no backward kernel): call it under torch.no_grad()')
    if q.dim() != 3 or kv.dim() != 3 or k2v2.dim() != 3:
        raise RuntimeError('cross_attention2: q, kv and k2v2 must be [B, tokens, channels]')
    B, Nq, C = q.shape
    es = q.element_size()
    sfx = '_ps' if (prescaled and q.dtype == BF16) else ''
    if prescaled and not sfx:
        raise RuntimeError('pre-scaled queries exist in the bf16 compute mode only')
    if heads <= 0 or C % heads:
        raise RuntimeError(f'cross_attention2: {heads} heads do not divide {C} channels')
    D = C // heads
    step = 4 if q.dtype == F32 else 8
    if D % step or D > 160:
        raise RuntimeError(f'cross_attention2: head width {D} is not admitted: it must be a multiple of {step} up to 160')
    if kv.shape[0] != B or kv.shape[2] != 2 * C:
        raise RuntimeError(f'cross_attention2: kv {tuple(kv.shape)}: expected [{B}, L, {2 * C}]')
    if tuple(k2v2.shape[::2]) != (B, 2 * C):
        raise RuntimeError(f'cross_attention2: k2v2 {tuple(k2v2.shape)}: expected [{B}, T, {2 * C}]')
    Nk, Nk2 = kv.shape[1], k2v2.shape[1]
    if not 1 <= Nk <= CROSS2_MAX_KEYS:
        raise RuntimeError(f'cross_attention2: {Nk} text keys: the kernel admits 1 .. {CROSS2_MAX_KEYS}')
    if not 1 <= Nk2 <= CROSS2_MAX_KEYS2:
        raise RuntimeError(f'cross_attention2: {Nk2} image keys: the kernel admits 1 .. {CROSS2_MAX_KEYS2}')
    ld2, bs2 = k2v2.stride(1), k2v2.stride(0)
    if k2v2.stride(2) != 1 or ld2 < 2 * C or (ld2 * es) % 16 or (bs2 * es) % 16 or (k2v2.data_ptr() % 16) or bs2 < 0:
        raise RuntimeError(f'cross_attention2: k2v2 strides {tuple(k2v2.stride())}: expected unit channel stride and 16-byte aligned rows, '
                           'batches and base address')
    if q.dtype == F32:
        r16 = lambda n: (n + 15) // 16 * 16      # noqa: E731
        need = 2 * (r16(Nk) + r16(Nk2)) * (r16(D) + 4) * 4
        if need > CROSS2_LDS_BYTES:
            raise RuntimeError(f'cross_attention2 (fp32): {Nk} + {Nk2} keys of width {D} need {need} bytes of LDS, more than {CROSS2_LDS_BYTES}')
    s = float(s)
    if s != s or s in (float('inf'), float('-inf')):
        raise RuntimeError(f'cross_attention2: scale {s} is not finite')
    o = torch.empty((B, Nq, C), device=q.device, dtype=q.dtype)
    _fn('attn_cross2_fwd' + sfx, q.dtype)(_p(q), _p(kv), kv.data_ptr() + C * es, k2v2.data_ptr(), k2v2.data_ptr() + C * es, _p(o), s,
                                        B, heads, Nq, Nk, Nk2, D, C, 2 * C, 2 * C, ld2, ld2, C, Nq * C, Nk * 2 * C, Nk * 2 * C, bs2, bs2, Nq * C, _s())
    return o


class _GEGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h):
        _chk(h, ACT)
        F2 = h.shape[-1]
        M = h.numel() // F2
        y = torch.empty(h.shape[:-1] + (F2 // 2,), device=h.device, dtype=h.dtype)
        _fn('geglu_fwd', h.dtype)(_p(h), _p(y), M, F2 // 2, _s())
        ctx.save_for_backward(h)
        return y

    @staticmethod
    def backward(ctx, dy):
        (h,) = ctx.saved_tensors
        F2 = h.shape[-1]
        dh = torch.empty_like(h)
        _fn('geglu_bwd', h.dtype)(_p(h), _p(dy.contiguous().to(h.dtype)), _p(dh), h.numel() // F2, F2 // 2, _s())
        return dh


def geglu(h):
    return _GEGLU.apply(h)


# A/B knob: smallest K at which the fused FF-in + GEGLU kernel is used when h is kept.  640 while the fusion lived on gemm_v3_kernel only (K = 320 with h: A-stationary
# GEMM + stand-alone GEGLU 164 + 87 us against 262 us fused, batch 16); 320 since the fusion runs on the 256 x 320 kernel (225-229 us: tools/geglu_p8_bench.py, round 6)
_GEGLU_FUSE_MIN_K = int(os.environ.get('SIDLSG_GEGLU_FUSE_MIN_K', '320'))


class _LinearGEGLU(torch.autograd.Function):
    """y = GEGLU(x W^T + b) with the projection and the gating in ONE kernel (sidlsg_gemm_geglu_bf16): the separate GEGLU pass over
    h = x W^T + b [M, 2F] -- at the 64x64 stage of SD1.5 a 335 MB read that took longer than the projection itself -- disappears.
    h is still written when a backward will need it (GEGLU's derivative needs both halves); under no_grad it is not even stored.
    Backward = sidlsg_geglu_bwd followed by the ordinary Linear backward (data gradient through w16t, weight + bias gradient)."""

    @staticmethod
    def forward(ctx, x, weight, bias, w16, w16t, keep_h, with_h=False):
        _chk(x, BF16)
        M, K = x.shape
        N2 = w16.shape[0]
        y = torch.empty((M, N2 // 2), device=x.device, dtype=BF16)
        h = torch.empty((M, N2), device=x.device, dtype=BF16) if keep_h else None
        lib.sidlsg_gemm_geglu_bf16(_p(x), x.stride(0), _p(w16), _p(h), N2, _p(y), N2 // 2, _p(bias), M, N2, K, _s())
        if keep_h:
            ctx.save_for_backward(x, weight, bias, w16t, h)
            ctx.masters = (weight, bias)
        if with_h:
            # h as a second output: the consumer (_GegluLinear) returns the gradient with respect to h itself -- its data-gradient
            # GEMM applies the GEGLU derivative in the epilogue -- and no gradient for y
            ctx.set_materialize_grads(False)
            return y, h
        return y

    @staticmethod
    def backward(ctx, dy, dh=None):
        x, _, _, w16t, h = ctx.saved_tensors
        weight, bias = ctx.masters
        F2 = h.shape[-1]
        if dy is not None:
            dh_y = torch.empty_like(h)
            lib.sidlsg_geglu_bwd(_p(h), _p(dy.contiguous().to(BF16)), _p(dh_y), h.shape[0], F2 // 2, _s())
            dh = dh_y if dh is None else add(dh.contiguous().to(BF16), dh_y)
        elif dh is None:
            return None, None, None, None, None, None, None
        else:
            dh = _gradc(dh)
        dx = gemm(dh, w16t) if ctx.needs_input_grad[0] else None
        if _wants_grad(weight):
            M, K = x.shape
            need_b = _wants_grad(bias)
            assign = _take_assign(weight, BF16)
            if not _queue_dense_wgrad(dh, x, weight.grad, bias.grad if need_b else None, M, weight.shape[0], K, assign, weight):
                wg = lib.sidlsg_wgrad_assign_bf16 if assign else lib.sidlsg_wgrad_bf16
                with _OnWgradStream(dh, x, dws=(weight.grad,)):
                    wg(_p(dh), dh.stride(0), _p(x), x.stride(0), _p(weight.grad), _p(bias.grad) if need_b else None, M, weight.shape[0], K, _s())
        elif _wants_grad(bias):
            colsum(dh, dh.shape[0], total=bias.grad)
        return dx, None, None, None, None, None, None


def linear_geglu(x, weight, bias, w16, w16t, with_h=False):
    """GEGLU(Linear(x)): the fused kernel where it applies (bf16, a shape the direct-to-LDS GEMM takes), else the two ops.
    with_h: return (y, h) -- h = None when no backward will run, y = None when the caller has to apply the GEGLU itself
    (feed_forward_out does, inside the node whose backward fuses the GEGLU derivative into the FF-out data gradient)."""
    if (_dual is None and x.dtype == BF16 and isinstance(w16, torch.Tensor) and w16.dtype == BF16 and x.is_contiguous()
            and lib.sidlsg_gemm_geglu_ok.raw(x.shape[0], w16.shape[0], w16.shape[1])):
        keep_h = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad))
        # measured (tools/ab/geglu_fused.py, MI355X, batch 16): K = 640 / 1280 (32x32 / 16x16 stages) 177 -> 165 us / 134 -> 120 us with h
        # kept; K = 320 (64x64 stage) only pays when h is NOT kept (251 -> 190 us): with h the A-stationary GEMM + the stand-alone
        # GEGLU kernel (164 + 87 us) beat the fused direct-to-LDS kernel (262 us); inside the step the two are equal (SIDLSG_GEGLU_FUSE_MIN_K=320
        # vs 640, eight alternations: 208.5 vs 208.7 ms, tools/_run50.sh)
        if not keep_h or w16.shape[1] >= _GEGLU_FUSE_MIN_K:
            if with_h and keep_h:
                return _LinearGEGLU.apply(x, weight, bias, w16, w16t, keep_h, True)
            y = _LinearGEGLU.apply(x, weight, bias, w16, w16t, keep_h)
            return (y, None) if with_h else y
    h = linear(x, weight, bias, w16, w16t)
    return (None, h) if with_h else geglu(h)


class _GegluLinear(torch.autograd.Function):
    """out = GEGLU(h) W^T + b (+ res): the GEGLU and the FF-out projection of a transformer block as ONE autograd node, so that the
    backward is sidlsg_gemm_geglu_bwd_bf16 -- the projection's data gradient with the GEGLU derivative in its epilogue: dy [M, F]
    is neither written nor re-read (2 x 168 MB at the 64x64 stage of SD1.5, batch 16) and sidlsg_geglu_bwd is not launched.
    y: GEGLU(h) when the fused FF-in kernel has already produced it (then no gradient flows back through y), else None."""

    @staticmethod
    def forward(ctx, h, y, weight, bias, w16, w16t, res):
        _chk(h, BF16)
        M, F2 = h.shape
        if y is None:
            y = torch.empty((M, F2 // 2), device=h.device, dtype=BF16)
            lib.sidlsg_geglu_fwd(_p(h), _p(y), M, F2 // 2, _s())
        out = gemm(y, w16, bias=bias, res=res)
        wg = weight.requires_grad
        ctx.save_for_backward(h, y if wg else None, weight, bias, w16t)
        ctx.masters = (weight, bias)
        ctx.has_res = res is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        h, y, _, _, w16t = ctx.saved_tensors
        weight, bias = ctx.masters
        dout = _gradc(dout)
        M, F2 = h.shape
        K = dout.shape[1]
        dh = None
        if ctx.needs_input_grad[0]:
            dh = torch.empty_like(h)
            lib.sidlsg_gemm_geglu_bwd_bf16(_p(dout), dout.stride(0), _p(w16t), _p(h), _p(dh), F2, M, F2 // 2, K, _s())
        need_b = _wants_grad(bias)
        if _wants_grad(weight):
            assign = _take_assign(weight, BF16)
            if not _queue_dense_wgrad(dout, y, weight.grad, bias.grad if need_b else None, M, weight.shape[0], F2 // 2, assign, weight):
                wgk = lib.sidlsg_wgrad_assign_bf16 if assign else lib.sidlsg_wgrad_bf16
                with _OnWgradStream(dout, y, dws=(weight.grad,)):
                    wgk(_p(dout), dout.stride(0), _p(y), y.stride(0), _p(weight.grad), _p(bias.grad) if need_b else None, M, weight.shape[0],
                        F2 // 2, _s())
        elif need_b:
            colsum(dout, dout.shape[0], total=bias.grad)
        dres = dout if (ctx.has_res and ctx.needs_input_grad[6]) else None
        return dh, None, None, None, None, None, dres


_FF_G2 = os.environ.get('SIDLSG_FF_G2', '1') != '0'      # A/B: the grouped pass's FeedForward as one node with the fused GEGLU kernels


class _FeedForwardG2(torch.autograd.Function):
    """The FeedForward block of the GROUPED frozen pass (two networks, stacked batch) as ONE autograd node over the grouped forms of the two
    GEGLU fusions: forward = sidlsg_gemm_geglu_bf16_g2 (FF-in projection + gating in one kernel; h is written only when a backward will need
    it) where the fused kernel pays -- K >= 640 with h kept, every admissible shape without -- else grouped GEMM + sidlsg_geglu_fwd, then the
    grouped FF-out GEMM (+ bias + residual); backward (data gradient only: both networks are frozen) = sidlsg_gemm_geglu_bwd_bf16_g2 (FF-out
    data gradient with the GEGLU derivative in its epilogue: dy [M, F] is neither written nor re-read) and the grouped FF-in data gradient.
    Until round 6 this pass -- 64 of an iteration's 144 sample-passes -- ran the unfused chain (grouped GEMMs + stand-alone GEGLU kernels),
    because the fusions only existed for single weight sets."""

    @staticmethod
    def forward(ctx, x, b1, w1_16, w1_16t, b2, w2_16, w2_16t, res, keep_h):
        _chk(x, BF16)
        M, K = x.shape
        N2 = w1_16[0].shape[0]
        F = N2 // 2
        ensure_workspace(x.device)
        y = torch.empty((M, F), device=x.device, dtype=BF16)
        h = None
        if x.is_contiguous() and lib.sidlsg_gemm_geglu_ok.raw(M, N2, K) and (not keep_h or K >= _GEGLU_FUSE_MIN_K):
            h = torch.empty((M, N2), device=x.device, dtype=BF16) if keep_h else None
            lib.sidlsg_gemm_geglu_bf16_g2(_p(x), x.stride(0), _p(w1_16[0]), _p(w1_16[1]), _p(h), N2, _p(y), F, _p(b1[0]), _p(b1[1]), M, N2, K, _s())
        else:
            h = gemm(x, w1_16, bias=b1)
            lib.sidlsg_geglu_fwd(_p(h), _p(y), M, F, _s())
            if not keep_h:
                h = None
        out = gemm(y, w2_16, bias=b2, res=res)
        ctx.save_for_backward(h)
        ctx.ops = (w1_16t, w2_16t)
        ctx.has_res = res is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        (h,) = ctx.saved_tensors
        w1_16t, w2_16t = ctx.ops
        dout = _gradc(dout)
        dx = None
        if ctx.needs_input_grad[0]:
            M, F2 = h.shape
            Kd = dout.shape[1]
            dh = torch.empty_like(h)
            if lib.sidlsg_gemm_geglu_bwd_ok.raw(M, F2 // 2, Kd):
                lib.sidlsg_gemm_geglu_bwd_bf16_g2(_p(dout), dout.stride(0), _p(w2_16t[0]), _p(w2_16t[1]), _p(h), _p(dh), F2, M, F2 // 2, Kd, _s())
            else:
                dy = gemm(dout, w2_16t)
                lib.sidlsg_geglu_bwd(_p(h), _p(dy), _p(dh), M, F2 // 2, _s())
            dx = gemm(dh, w1_16t)
        dres = dout if (ctx.has_res and ctx.needs_input_grad[7]) else None
        return dx, None, None, None, None, None, None, dres, None


def feed_forward(x, w1, b1, w1_16, w1_16t, w2, b2, w2_16, w2_16t, res=None):
    """diffusers FeedForward (GEGLU projection -> Linear) + the block's residual: out = GEGLU(x W1^T + b1) W2^T + b2 + res."""
    if (_dual is not None and _FF_G2 and x.dtype == BF16 and isinstance(w1_16, torch.Tensor) and w1_16.dtype == BF16
            and isinstance(w2_16, torch.Tensor) and w2_16.dtype == BF16 and b1 is not None and b2 is not None and w1_16.shape[0] % 2 == 0
            and x.shape[0] % 2 == 0):
        _frozen(_pair(w1), _pair(b1), _pair(w2), _pair(b2))
        keep_h = torch.is_grad_enabled() and x.requires_grad      # (grad mode is off inside Function.forward: decided here)
        return _FeedForwardG2.apply(x, _pair(b1), _pair(w1_16), _pair(w1_16t), _pair(b2), _pair(w2_16), _pair(w2_16t), res, keep_h)
    fused_bwd = (_dual is None and x.dtype == BF16 and torch.is_grad_enabled() and isinstance(w2_16, torch.Tensor) and w2_16.dtype == BF16
                 and isinstance(w1_16, torch.Tensor)
                 and lib.sidlsg_gemm_geglu_bwd_ok.raw(x.shape[0], w2_16.shape[1], w2_16.shape[0]))
    if not fused_bwd:
        return linear(linear_geglu(x, w1, b1, w1_16, w1_16t), w2, b2, w2_16, w2_16t, res)
    y, h = linear_geglu(x, w1, b1, w1_16, w1_16t, with_h=True)
    return geglu_linear(h, y, w2, b2, w2_16, w2_16t, res)


def geglu_linear(h, y, weight, bias, w16, w16t, res=None):
    """GEGLU(h) -> Linear (+ res) with the fused backward where it applies; h = None: y is all there is (no backward will run)."""
    if h is None:
        return linear(y, weight, bias, w16, w16t, res)
    if (_dual is None and h.dtype == BF16 and h.requires_grad and torch.is_grad_enabled() and isinstance(w16, torch.Tensor) and w16.dtype == BF16
            and h.is_contiguous() and lib.sidlsg_gemm_geglu_bwd_ok.raw(h.shape[0], h.shape[1] // 2, w16.shape[0])):
        return _GegluLinear.apply(h, y, weight, bias, w16, w16t, res)
    return linear(y if y is not None else geglu(h), weight, bias, w16, w16t, res)


class _SiLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x, ACT)
        y = torch.empty_like(x)
        _fn('silu_fwd', x.dtype)(_p(x), _p(y), x.numel(), _s())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        _fn('silu_bwd', x.dtype)(_p(x), _p(dy.contiguous().to(x.dtype)), _p(dx), x.numel(), _s())
        return dx


def silu(x):
    return _SiLU.apply(x)


class _Concat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _chk(a, ACT)
        _chk(b, a.dtype)
        C1, C2 = a.shape[-1], b.shape[-1]
        M = a.numel() // C1
        out = torch.empty(a.shape[:-1] + (C1 + C2,), device=a.device, dtype=a.dtype)
        _fn('concat2', a.dtype)(_p(a), _p(b), _p(out), M, C1, C2, 0, _s())
        ctx.shapes = (a.shape, b.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        sa, sb = ctx.shapes
        g = g.contiguous()
        da = torch.empty(sa, device=g.device, dtype=g.dtype)
        db = torch.empty(sb, device=g.device, dtype=g.dtype)
        _fn('concat2', g.dtype)(_p(da), _p(db), _p(g), da.numel() // sa[-1], sa[-1], sb[-1], 1, _s())
        return da, db


def concat_channels(a, b):
    return _Concat.apply(a, b)


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        o = torch.empty_like(a)
        _fn('add', a.dtype, '_bf16')(_p(_chk(a, ACT)), _p(_chk(b, a.dtype)), _p(o), a.numel(), _s())
        return o

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return _Add.apply(a, b)


def timestep_embed(t, dim, dtype=BF16):
    out = torch.empty((t.shape[0], dim), device=t.device, dtype=dtype)
    _fn('timestep_embed', dtype)(_p(_chk(t, torch.int64)), _p(out), t.shape[0], dim, _s())
    return out


# ------------------------------------------------------------------------------------------------
# scheduler / guidance glue and losses
class _NoisyInput(torch.autograd.Function):
    """x_t = s0*x0 + s1*noise -> (NHWC activations [dup*B,H,W,8] of `dtype`, x_t fp32 NCHW).  x0 may be None."""

    @staticmethod
    def forward(ctx, x0, noise, s0, s1, dup, dtype):
        B, C, H, W = noise.shape
        out = torch.empty((dup * B, H, W, 8), device=noise.device, dtype=dtype)
        xt = torch.empty_like(noise)
        _fn('noisy_input', dtype)(_p(x0), _p(_chk(noise, F32)), _p(s0), _p(s1), _p(out), _p(xt), B, C, H * W, 8, dup, _s())
        ctx.save_for_backward(s0, s1)
        ctx.cfg = (B, C, H, W, dup)
        return out, xt

    @staticmethod
    def backward(ctx, g, gxt):
        s0, s1 = ctx.saved_tensors
        B, C, H, W, dup = ctx.cfg
        g = g.contiguous()
        outs = []
        for idx, sc in ((0, s0), (1, s1)):
            if not ctx.needs_input_grad[idx]:
                outs.append(None)
                continue
            d = torch.empty((B, C, H, W), device=g.device, dtype=F32)
            _fn('noisy_input_bwd', g.dtype)(_p(g), _p(sc), _p(d), B, C, H * W, 8, dup, 0, _s())
            if gxt is not None:
                d = d + gxt * sc.view(B, 1, 1, 1)
            outs.append(d)
        return outs[0], outs[1], None, None, None, None


def noisy_input(x0, noise, s0, s1, dup, dtype=BF16):
    return _NoisyInput.apply(x0, noise, s0, s1, dup, dtype)


class _CfgX0(torch.autograd.Function):
    """eps [dup*B,HW,C] fp32 (+ x_t) -> NCHW fp32 guided output (mode 0) or x0 prediction (mode 1: epsilon, 2: v)."""

    @staticmethod
    def forward(ctx, eps, xt, s0, s1, kappa, mode, act_dtype):
        B, C, H, W = xt.shape
        dup = eps.shape[0] // B
        out = torch.empty_like(xt)
        lib.sidlsg_cfg_x0(_p(_chk(eps, F32)), _p(_chk(xt, F32)), _p(s0), _p(s1), _p(out), B, C, H * W, eps.shape[-1], dup,
                          float(kappa), mode, _s())
        ctx.save_for_backward(s0, s1)
        ctx.cfg = (B, C, H, W, dup, float(kappa), mode, act_dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        s0, s1 = ctx.saved_tensors
        B, C, H, W, dup, kappa, mode, act_dtype = ctx.cfg
        deps = torch.empty((dup * B, H * W, 8), device=g.device, dtype=act_dtype)    # the network's activation dtype
        dxt = torch.empty((B, C, H, W), device=g.device, dtype=F32) if ctx.needs_input_grad[1] else None
        _fn('cfg_x0_bwd', act_dtype)(_p(g.contiguous()), _p(s0), _p(s1), _p(deps), _p(dxt), B, C, H * W, 8, dup, kappa, mode, _s())
        return deps, dxt, None, None, None, None, None


def cfg_x0(eps, xt, s0, s1, kappa, predict_x0, act_dtype=BF16, prediction_type='epsilon'):
    """u + kappa (c - u), then (predict_x0) x0 under the network's parameterisation `prediction_type` ('epsilon' | 'v_prediction');
    predict_x0 False returns the guided network output itself."""
    mode = prediction_mode(prediction_type) if predict_x0 else 0
    return _CfgX0.apply(eps, xt, s0, s1, kappa, mode, act_dtype)


class _StepRenoise(torch.autograd.Function):
    """One step boundary of the multi-step generator (sidlsg_step_renoise): the generator output eps [B,HW,8] fp32 at t_i and x_{t_i}
    -> x_hat (x0 prediction, mode 1 epsilon / 2 v) -> x_{t_{i+1}} = s0n*x_hat + s1n*noise, returned as (NHWC activations [B,H,W,8] of
    `dtype`, x_{t_{i+1}} fp32 NCHW).  Forward bit-equal to cfg_x0(..., True) followed by noisy_input(x_hat, noise, s0n, s1n, 1)."""

    @staticmethod
    def forward(ctx, eps, xt, s0, s1, s0n, s1n, noise, mode, dtype):
        B, C, H, W = xt.shape
        if tuple(eps.shape) != (B, H * W, 8) or tuple(noise.shape) != tuple(xt.shape):
            raise RuntimeError(f'step_renoise: eps {tuple(eps.shape)} / noise {tuple(noise.shape)} do not match x_t {tuple(xt.shape)}')
        out = torch.empty((B, H, W, 8), device=xt.device, dtype=dtype)
        xtn = torch.empty_like(xt)
        _fn('step_renoise', dtype)(_p(_chk(eps, F32)), _p(_chk(xt, F32)), _p(s0), _p(s1), _p(s0n), _p(s1n), _p(_chk(noise, F32)),
                                   _p(out), _p(xtn), B, C, H * W, 8, mode, _s())
        ctx.save_for_backward(s0, s1, s0n)
        ctx.cfg = (B, C, H, W, mode, dtype)
        return out, xtn

    @staticmethod
    def backward(ctx, g, gxtn):
        s0, s1, s0n = ctx.saved_tensors
        B, C, H, W, mode, dtype = ctx.cfg
        g = g.contiguous()
        if g.dtype != dtype:
            g = g.to(dtype)
        gxtn = gxtn.contiguous() if gxtn is not None else None
        deps = torch.empty((B, H * W, 8), device=g.device, dtype=dtype)      # the network's activation dtype (as _CfgX0)
        dxt = torch.empty((B, C, H, W), device=g.device, dtype=F32) if ctx.needs_input_grad[1] else None
        _fn('step_renoise_bwd', dtype)(_p(g), _p(gxtn), _p(s0), _p(s1), _p(s0n), _p(deps), _p(dxt), B, C, H * W, 8, mode, _s())
        return deps, dxt, None, None, None, None, None, None, None


def step_renoise(eps, xt, s0, s1, s0n, s1n, noise, act_dtype=BF16, prediction_type='epsilon'):
    """x_hat of step i (coefficients s0, s1 of t_i) re-noised to t_{i+1} (s0n, s1n) with `noise`: -> (next input, x_{t_{i+1}})."""
    return _StepRenoise.apply(eps, xt, s0, s1, s0n, s1n, noise, prediction_mode(prediction_type), act_dtype)


def ddim_step(eps, xt, s0, s1, s0p, s1p, kappa, act_dtype=BF16, prediction_type='epsilon', last=False, want_x0=False):
    """One step boundary of the teacher's deterministic DDIM sampler (sidlsg_ddim_step): the teacher's output eps [dup*B,HW,Ce] fp32
    at t ([uncond ; cond] when dup = 2) and x_t fp32 NCHW -> guided e, x0 prediction, x_prev = s0p*x0 + s1p*eps_hat with the
    coefficients (s0p, s1p) of the previous timestep.  Returns (next network input NHWC [dup*B,H,W,8] of `act_dtype`, or None when
    `last`; x_prev fp32 NCHW; the x0 prediction fp32 NCHW, or None unless `want_x0`).  Forward only."""
    if torch.is_grad_enabled() and any(torch.is_tensor(v) and v.requires_grad for v in (eps, xt, s0, s1, s0p, s1p)):
        raise RuntimeError('ddim_step is forward only: call it under torch.no_grad() (the teacher sampler is not differentiated)')
    B, C, H, W = xt.shape
    if eps.dim() != 3 or eps.shape[1] != H * W or eps.shape[0] not in (B, 2 * B) or eps.shape[2] < C:
        raise RuntimeError(f'ddim_step: eps {tuple(eps.shape)} does not match x_t {tuple(xt.shape)}')
    for name, v in (('s0', s0), ('s1', s1), ('s0p', s0p), ('s1p', s1p)):
        if v.numel() != B:
            raise RuntimeError(f'ddim_step: {name} has {v.numel()} elements, the batch has {B}')
    dup = eps.shape[0] // B
    out = None if last else torch.empty((dup * B, H, W, 8), device=xt.device, dtype=act_dtype)
    xtn = torch.empty_like(xt)
    x0 = torch.empty_like(xt) if want_x0 else None
    _fn('ddim_step', act_dtype)(_p(_chk(eps, F32)), _p(_chk(xt, F32)), _p(_chk(s0, F32)), _p(_chk(s1, F32)), _p(_chk(s0p, F32)),
                                _p(_chk(s1p, F32)), _p(out), _p(xtn), _p(x0), B, C, H * W, eps.shape[2], 8, dup, float(kappa),
                                prediction_mode(prediction_type), _s())
    return out, xtn, x0


solver_launches = dict(solver_step=0, cfg_rescale_stats=0, masked_renoise=0)   # launches issued through the wrappers below (tests count them)


def cfg_rescale_stats(eps, channels, kappa, phi):
    """The per-sample guidance-rescale factors of Lin et al. 2024 (sidlsg_cfg_rescale_stats): eps [2*B,HW,Ce] fp32 ([uncond ; cond])
    -> scale [B] fp32 = phi*std(c)/std(g) + 1 - phi, g = u + kappa*(c - u), the unbiased standard deviations over the `channels`
    real channels of a sample (centred, fixed summation order; std(g) = 0 gives 1).  Forward only."""
    if torch.is_grad_enabled() and eps.requires_grad:
        raise RuntimeError('cfg_rescale_stats is forward only: call it under torch.no_grad() (the teacher sampler is not differentiated)')
    if eps.dim() != 3 or eps.shape[0] % 2 or eps.shape[2] < channels:
        raise RuntimeError(f'cfg_rescale_stats: eps {tuple(eps.shape)} is not a [2*B, HW, >={channels}] pair of halves')
    B = eps.shape[0] // 2
    scale = torch.empty(B, device=eps.device, dtype=F32)
    lib.sidlsg_cfg_rescale_stats(_p(_chk(eps, F32)), _p(scale), B, int(channels), eps.shape[1], eps.shape[2], float(kappa), float(phi), _s())
    solver_launches['cfg_rescale_stats'] += 1
    return scale


def solver_step(eps, xt, s0, s1, coef, kappa, act_dtype=BF16, prediction_type='epsilon', x0p=None, noise=None, scale=None, last=False,
                x0_out=None, need_prev=None):
    """One step boundary of the teacher's solver family (sidlsg_solver_step): the teacher's output eps [dup*B,HW,Ce] fp32 at s
    ([uncond ; cond] when dup = 2) and x_s fp32 NCHW -> guided e (times `scale` [B] when given: ops.cfg_rescale_stats), x0 prediction,
    x_t = c_x*x_s + c_cur*x0 + c_prev*x0p + c_n*noise with coef [B,4] = (c_x, c_cur, c_prev, c_n) of scheduler.solver_schedule, x0p
    the x0 prediction of the step before and noise fresh N(0, 1) values (both fp32 NCHW, both optional: an absent term is not formed).
    `need_prev`: whether this step's c_prev is non-zero (the coefficients are on the device and are not read back); default: whether
    x0p was given.  True without x0p is refused by the kernel's host side.  `x0_out`: a buffer for the x0 prediction (the sampler
    ping-pongs two), else a new tensor.
    Returns (next network input NHWC [dup*B,H,W,8] of `act_dtype`, or None when `last`; x_t fp32 NCHW; the x0 prediction fp32 NCHW).
    Forward only."""
    tensors = (eps, xt, s0, s1, coef, x0p, noise, scale)
    if torch.is_grad_enabled() and any(torch.is_tensor(v) and v.requires_grad for v in tensors):
        raise RuntimeError('solver_step is forward only: call it under torch.no_grad() (the teacher sampler is not differentiated)')
    B, C, H, W = xt.shape
    if eps.dim() != 3 or eps.shape[1] != H * W or eps.shape[0] not in (B, 2 * B) or eps.shape[2] < C:
        raise RuntimeError(f'solver_step: eps {tuple(eps.shape)} does not match x_t {tuple(xt.shape)}')
    for name, v, n in (('s0', s0, B), ('s1', s1, B), ('coef', coef, 4 * B), ('scale', scale, B)):
        if v is not None and v.numel() != n:
            raise RuntimeError(f'solver_step: {name} has {v.numel()} elements, expected {n} for a batch of {B}')
    for name, v in (('x0p', x0p), ('noise', noise), ('x0_out', x0_out)):
        if v is not None and tuple(v.shape) != tuple(xt.shape):
            raise RuntimeError(f'solver_step: {name} {tuple(v.shape)} does not match x_t {tuple(xt.shape)}')
    dup = eps.shape[0] // B
    out = None if last else torch.empty((dup * B, H, W, 8), device=xt.device, dtype=act_dtype)
    xtn = torch.empty_like(xt)
    x0 = torch.empty_like(xt) if x0_out is None else x0_out
    opt = lambda v: None if v is None else _chk(v, F32)  # noqa: E731
    _fn('solver_step', act_dtype)(_p(_chk(eps, F32)), _p(_chk(xt, F32)), _p(_chk(s0, F32)), _p(_chk(s1, F32)), _p(_chk(coef, F32)),
                                  _p(opt(x0p)), _p(opt(noise)), _p(opt(scale)), _p(out), _p(xtn), _p(_chk(x0, F32)), B, C, H * W,
                                  eps.shape[2], 8, dup, float(kappa), prediction_mode(prediction_type),
                                  int(x0p is not None if need_prev is None else need_prev), _s())
    solver_launches['solver_step'] += 1
    return out, xtn, x0


def masked_renoise(x, z0, mask, noise=None, a0=None, a1=None, dup=1, act_dtype=BF16, want_input=True, inplace=False, cp=8):
    """The masked step boundary of inpainting (sidlsg_masked_renoise): x fp32 NCHW is what a sampler step produced at its target level,
    z0 the scaled init latents, `mask` uint8 / bool [B,h,w] or [1,h,w] (nonzero: repaint), noise the initial noise and a0 / a1 [B] the
    coefficients of the target level: known = a0*z0 + a1*noise with the roundings of noisy_input (a0 None means 1; without noise and
    a0, z0 itself), x_n = mask ? x : known -- a select.  `inplace` writes x_n over x.  Returns (next network input NHWC
    [dup*B,h,w,cp] of `act_dtype` -- the bits of noisy_input(None, x_n, 1, 1, dup) -- or None unless `want_input`; x_n fp32 NCHW).
    Forward only."""
    tensors = (x, z0, noise, a0, a1)
    if torch.is_grad_enabled() and any(torch.is_tensor(v) and v.requires_grad for v in tensors):
        raise RuntimeError('masked_renoise is forward only: call it under torch.no_grad() (the masked samplers are not differentiated)')
    if x.dim() != 4:
        raise RuntimeError(f'masked_renoise: x {tuple(x.shape)} is not [B, C, h, w]')
    B, C, H, W = x.shape
    for name, v in (('z0', z0), ('noise', noise)):
        if v is not None and tuple(v.shape) != tuple(x.shape):
            raise RuntimeError(f'masked_renoise: {name} {tuple(v.shape)} does not match x {tuple(x.shape)}')
    if mask.dtype not in (torch.uint8, torch.bool) or mask.dim() != 3 or tuple(mask.shape[1:]) != (H, W) or mask.shape[0] not in (1, B):
        raise RuntimeError(f'masked_renoise: mask {tuple(mask.shape)} {mask.dtype} is not a uint8 / bool [{B} or 1, {H}, {W}]')
    for name, v in (('a0', a0), ('a1', a1)):
        if v is not None and v.numel() != B:
            raise RuntimeError(f'masked_renoise: {name} has {v.numel()} elements, the batch has {B}')
    if (noise is None) != (a1 is None):
        raise RuntimeError('masked_renoise: noise and a1 are given together or not at all')
    m = _chk(mask, mask.dtype)
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    shared = int(mask.shape[0] == 1 and B > 1)
    out = torch.empty((dup * B, H, W, cp), device=x.device, dtype=act_dtype) if want_input else None
    xn = x if inplace else torch.empty_like(x)
    opt = lambda v: None if v is None else _chk(v, F32)  # noqa: E731
    _fn('masked_renoise', act_dtype)(_p(_chk(x, F32)), _p(_chk(z0, F32)), _p(opt(noise)), _p(m), _p(opt(a0)), _p(opt(a1)), _p(out), _p(xn),
                                     B, C, H * W, int(cp), int(dup), shared, _s())
    solver_launches['masked_renoise'] += 1
    return out, xn


class _GLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, yr, yf, alpha, scale):
        S = x.shape[0]
        n = x.numel() // S
        dx, dyr, dyf = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        loss = torch.empty(1, device=x.device, dtype=F32)
        ws = torch.empty(10 * S, device=x.device, dtype=F32)
        lib.sidlsg_g_loss(_p(_chk(x, F32)), _p(_chk(yr, F32)), _p(_chk(yf, F32)), _p(dx), _p(dyr), _p(dyf), _p(loss), _p(ws), S, n,
                          float(alpha), float(scale), _s())
        ctx.save_for_backward(dx, dyr, dyf)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        dx, dyr, dyf = ctx.saved_tensors
        return dx * g, dyr * g, dyf * g, None, None


def sid_generator_loss(x, y_real, y_fake, alpha, scale):
    return _GLoss.apply(x, y_real, y_fake, alpha, scale)


class _FakeLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, noise, scale):
        S = e.shape[0]
        n = e.numel() // S
        de = torch.empty_like(e)
        loss = torch.empty(1, device=e.device, dtype=F32)
        ws = torch.empty(10 * S, device=e.device, dtype=F32)
        lib.sidlsg_fake_loss(_p(_chk(e, F32)), _p(_chk(noise, F32)), _p(de), _p(loss), _p(ws), S, n, float(scale), _s())
        ctx.save_for_backward(de)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (de,) = ctx.saved_tensors
        return de * g, None, None


def sid_fake_score_loss(e, noise, scale):
    return _FakeLoss.apply(e, noise, scale)


class _FakeLossV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o, images, noise, s0, s1, w, scale):
        S = o.shape[0]
        n = o.numel() // S
        de = torch.empty_like(o)
        loss = torch.empty(1, device=o.device, dtype=F32)
        ws = torch.empty(10 * S, device=o.device, dtype=F32)
        lib.sidlsg_fake_loss_v(_p(_chk(o, F32)), _p(_chk(images, F32)), _p(_chk(noise, F32)), _p(_chk(s0, F32)), _p(_chk(s1, F32)),
                               _p(_chk(w, F32)), _p(de), _p(loss), _p(ws), S, n, float(scale), _s())
        ctx.save_for_backward(de)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (de,) = ctx.saved_tensors
        return de * g, None, None, None, None, None, None


def sid_fake_score_loss_v(o, images, noise, s0, s1, w, scale):
    """v-prediction fake-score loss: scale * sum_b w_b |o_b - v*_b|^2, v* = s0 noise - s1 images (never materialised), samples whose
    o or v* holds a NaN dropped.  Gradient to o only (`images` come from the generator's no-grad pass)."""
    return _FakeLossV.apply(o, images, noise, s0, s1, w, scale)


# ------------------------------------------------------------------------------------------------
def transpose_w(src_f32, n, k, taps=1, dtype=BF16):
    """fp32 master [N][T][K] -> [K][T reversed][N] of the compute dtype (the dgrad operand)"""
    dst = torch.empty((k, taps * n), device=src_f32.device, dtype=dtype)
    _fn('transpose_w', dtype)(_p(src_f32), _p(dst), n, k, taps, _s())
    return dst


class _ColumnGrads:
    """The gradient of a split_columns() source, built in place: one [n, sum C] fp32 buffer per backward pass (zeroed ONCE, on
    first use) into whose column slices the consumers' backward kernels accumulate (ops.colsum(slot=...)); _SplitColumns.backward
    hands it on as it is.  22 fills + a concat kernel per pass become one fill.

    Consumers of several live passes may accumulate into one buffer (a re-entrant pass in the middle of the outer one: a checkpointed
    consumer).  If any pass that accumulated into it raises, the buffer is dropped with that pass (the ledger `_passes`): the partial
    sums of a pass that died must not reach the next one."""

    def __init__(self, sizes):
        self.total, self.buf = sum(sizes), None

    def buffer(self, n, device):
        if _passes.once(('column grads', id(self))) and _passes.current() >= 0:
            _passes.on_death(functools.partial(_ColumnGrads._forget, weakref.ref(self)))
        if self.buf is None:
            self.buf = torch.zeros((n, self.total), device=device, dtype=F32)
        return self.buf if self.buf.shape[0] == n else None

    @staticmethod
    def _forget(ref):
        holder = ref()
        if holder is not None:
            holder.buf = None

    def take(self):
        b, self.buf = self.buf, None
        return b


class _SplitColumns(torch.autograd.Function):
    """x [N, sum C] -> views x[:, off_i:off_i+C_i] (no copies); backward = the shared column-gradient buffer when every part's
    gradient is its slice of it (the normal case), else one torch.cat of the column gradients."""

    @staticmethod
    def forward(ctx, x, sizes, holder):
        ctx.sizes, ctx.meta, ctx.holder = sizes, (x.shape[0], x.dtype, x.device), holder
        return tuple(x.split(sizes, dim=1))

    @staticmethod
    def backward(ctx, *grads):
        n, dtype, dev = ctx.meta
        buf = ctx.holder.take()
        if buf is not None and dtype == F32 and buf.shape[0] == n:
            off, ok = 0, True
            for g, c in zip(grads, ctx.sizes):
                ok = ok and g is not None and g.dtype == F32 and g.data_ptr() == buf.data_ptr() + 4 * off and g.stride(0) == buf.stride(0) and g.shape == (n, c)
                off += c
            if ok:
                return buf, None, None
        gs = [g if g is not None else torch.zeros((n, c), device=dev, dtype=dtype) for g, c in zip(grads, ctx.sizes)]
        return torch.cat([g.to(dtype) for g in gs], dim=1), None, None


def split_columns(x, sizes):
    """-> tuple of column views; part._col_slot = (holder, offset, width) lets a consumer's backward accumulate its gradient in place."""
    sizes = list(sizes)
    holder = _ColumnGrads(sizes)
    parts = _SplitColumns.apply(x, sizes, holder)
    off = 0
    for p, c in zip(parts, sizes):
        p._col_slot = (holder, off, c)
        off += c
    return parts


class _GradReady(torch.autograd.Function):
    """Identity whose backward calls `cb()` before passing the gradient on: placed at a block boundary in the forward, it
    fires when the backward has finished everything AFTER that boundary (autograd runs ready nodes with the highest
    sequence number first, and the marker is older than every node of the blocks behind it)."""

    @staticmethod
    def forward(ctx, x, cb):
        ctx.cb = cb
        return x.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        flush_deferred()        # queued dgamma / dbeta reductions belong to the segment that is about to be declared final
        ctx.cb()
        return g, None


def grad_ready_marker(x, cb):
    return _GradReady.apply(x, cb) if (cb is not None and x.requires_grad) else x


class _AfterBackward(torch.autograd.Function):
    """Identity on the network output; its backward (the FIRST node of that network's backward) queues `cb` on the
    autograd engine, which runs it once the whole backward pass has finished."""

    @staticmethod
    def forward(ctx, x, cb):
        ctx.cb = cb
        return x.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        torch.autograd.Variable._execution_engine.queue_callback(ctx.cb)
        return g, None


def after_backward(x, cb):
    return _AfterBackward.apply(x, cb) if x.requires_grad else x


def transpose_w_batched(jobs, njobs, nblocks, dtype=BF16, src16=False):
    """jobs: device uint8 tensor holding njobs sidlsg_tw_job records (see include/sidlsg_hip.h); dtype: of the destinations;
    src16: the records' sources are the bf16 compute copies (64x64-tile job table)."""
    if src16:
        lib.sidlsg_transpose_w16_batched(_p(jobs), njobs, nblocks, _s())
    else:
        _fn('transpose_w_batched', dtype)(_p(jobs), njobs, nblocks, _s())


def scale_cast_ranges(jobs, njobs, nblocks):
    """jobs: device uint8 tensor of njobs records (include/sidlsg_hip.h): dst = bf16(scale * src) per range."""
    lib.sidlsg_scale_cast_ranges(_p(jobs), njobs, nblocks, _s())


LORA_JOB_DTYPE = [('base', '<u8'), ('dst', '<u8'), ('up', '<u8'), ('down', '<u8'), ('coef', '<u8'),
                  ('N', '<i4'), ('KK', '<i4'), ('R', '<i4'), ('blk0', '<i4')]
LORA_TILE = 64
LORA_MAX_RANK = 4096


class LoraJobTable:
    """The job table of sidlsg_lora_merge_f32 (include/sidlsg_hip.h): `records` is a sequence of (base, dst, up, down, coef, N, KK, R)
    with the five operands as device pointers; blk0 is filled in here (64 x 64 tiles, in order, gap-free).  Holds the host copy the
    entry point validates and the device copy the kernel reads."""

    def __init__(self, records, device):
        import numpy as np
        rec = np.zeros(len(records), dtype=np.dtype(LORA_JOB_DTYPE))
        blk = 0
        for i, (base, dst, up, down, coef, n, kk, r) in enumerate(records):
            rec[i] = (base, dst, up, down, coef, n, kk, r, blk)
            blk += -(-n // LORA_TILE) * -(-kk // LORA_TILE)
        self.host = rec
        self.njobs, self.nblocks = len(records), blk
        self.device = torch.from_numpy(rec.view(np.uint8).copy()).to(device) if len(records) else None


def lora_merge(table, names=None):
    """One launch: dst = base + (coef * up) @ down for every job of `table` (LoraJobTable).  A record outside the admitted shapes
    raises a ValueError that names the layer (`names`: one per job), before anything is launched."""
    if table.njobs == 0:
        return
    fault = lora_job_fault(table.host, table.nblocks, names)
    if fault is not None:
        raise ValueError('LoRA merge job table: ' + fault)
    lib.sidlsg_lora_merge_f32(table.host.ctypes.data, _p(table.device), table.njobs, table.nblocks, _s())


def lora_job_fault(rec, nblocks, names=None):
    """The Python side's ONE check of a LoRA job table against the contract of sidlsg_lora_merge_f32 (include/sidlsg_hip.h), run before
    every launch: None when the table is admitted, else which record breaks which rule, in words.  The entry point checks again and
    answers SIDLSG_EINVAL; a table that passes here and fails there is a disagreement between the two and surfaces as the binding's
    RuntimeError with the code."""
    blk = 0
    for i, r in enumerate(rec):
        who = names[i] if names else f'job {i}'
        n, kk, rr = int(r['N']), int(r['KK']), int(r['R'])
        for f in ('base', 'dst', 'up', 'down', 'coef'):
            if int(r[f]) == 0 or int(r[f]) % 16:
                return f'{who}: {f} pointer {int(r[f]):#x} is null or not 16-byte aligned'
        if n < 1 or kk < 4 or kk % 4:
            return f'{who}: weight [{n}][{kk}]: needs N >= 1 and a row length that is a multiple of 4'
        if rr < 4 or rr % 4 or rr > LORA_MAX_RANK:
            return f'{who}: concatenated rank {rr}: needs a multiple of 4 in [4, {LORA_MAX_RANK}]'
        if n * kk * 4 >= 1 << 31:
            return f'{who}: weight [{n}][{kk}] is 2^31 bytes or more'
        if int(r['blk0']) != blk:
            return f'{who}: blk0 {int(r["blk0"])} out of sequence (expected {blk})'
        blk += -(-n // LORA_TILE) * -(-kk // LORA_TILE)
    if blk != nblocks:
        return f'nblocks {nblocks} is not the total {blk}'
    return None


def cast_bf16(src_f32, out=None):
    if out is None:
        out = torch.empty(src_f32.shape, device=src_f32.device, dtype=BF16)
    lib.sidlsg_cast_f32_bf16(_p(src_f32), _p(out), src_f32.numel(), _s())
    return out


def image_grid_u8(images, grid, first, gw, drange=(-1, 1), layout='nchw'):
    """Place decoded fp32 images into their tiles of the uint8 preview grid `grid` [gh*H, gw*W, 3] (sidlsg_image_grid_u8): image i
    goes to tile first + i (row-major, gw tiles per row).  layout 'nhwc8': images [B, H, W, 8], channels 3..7 padding (the VAE
    decoder's native output); 'nchw': [B, 3, H, W] (sid_sd_sampler(return_images=True)).  uint8 = clip(rint((x - lo) * 255 / (hi - lo)))
    in fp32 with numpy's roundings (save_image_grid, sid_training_loop.py:99-103)."""
    if layout == 'nhwc8':
        B, H, W, C = images.shape
        ok = C == 8
    elif layout == 'nchw':
        B, C, H, W = images.shape
        ok = C == 3
    else:
        raise ValueError(f"image_grid_u8: layout {layout!r}: expected 'nhwc8' or 'nchw'")
    if not ok:
        raise RuntimeError(f'image_grid_u8: images {tuple(images.shape)} are not {layout}')
    if grid.dim() != 3 or grid.shape[2] != 3 or grid.shape[1] != gw * W or grid.shape[0] % H:
        raise RuntimeError(f'image_grid_u8: grid {tuple(grid.shape)} is not [gh*{H}, {gw}*{W}, 3]')
    lo, hi = drange
    lib.sidlsg_image_grid_u8(_p(_chk(images, F32)), _p(_chk(grid, torch.uint8)), B, H, W, 1 if layout == 'nchw' else 0, int(first), int(gw),
                             grid.shape[0] // H, float(lo), float(hi), _s())
    return grid


def image_to_nhwc8(images):
    """Images -> the [B, H, W, 8] bf16 NHWC activation the VAE encoder's conv_in takes, channels 3..7 zero (sidlsg_image_to_nhwc8).
    uint8 [B, H, W, 3]: x / 127.5 - 1 in fp32 (IEEE division, subtraction), rounded to bf16; fp32 [B, 3, H, W] in [-1, 1]: rounded."""
    if images.dtype == torch.uint8 and images.dim() == 4 and images.shape[3] == 3:
        B, H, W, _ = images.shape
        out = torch.empty((B, H, W, 8), device=images.device, dtype=BF16)
        lib.sidlsg_image_to_nhwc8(_p(_chk(images, torch.uint8)), _p(out), B, H, W, _s())
    elif images.dtype == F32 and images.dim() == 4 and images.shape[1] == 3:
        B, _, H, W = images.shape
        out = torch.empty((B, H, W, 8), device=images.device, dtype=BF16)
        lib.sidlsg_image_to_nhwc8_f32(_p(_chk(images, F32)), _p(out), B, H, W, _s())
    else:
        raise RuntimeError(f'image_to_nhwc8: expected uint8 [B, H, W, 3] or fp32 [B, 3, H, W], got {images.dtype} {tuple(images.shape)}')
    return out


def control_hint_u8(images, dtype=BF16):
    """Control images uint8 [B, H, W, 3] (RGB) -> the ControlNet hint embedder's input [B, H, W, 8] of `dtype` (bf16 or fp32), channels 3..7
    zero (sidlsg_control_hint_u8): float(x) / 255, one IEEE fp32 division, rounded to nearest even for bf16 -- the bits of
    (images.float() / 255).to(dtype) formed on the host."""
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise RuntimeError(f'control_hint_u8: expected uint8 [B, H, W, 3], got {images.dtype} {tuple(images.shape)}')
    if dtype not in (BF16, F32):
        raise RuntimeError(f'control_hint_u8: output dtype {dtype}: expected bfloat16 or float32')
    B, H, W, _ = images.shape
    out = torch.empty((B, H, W, 8), device=images.device, dtype=dtype)
    lib.sidlsg_control_hint_u8(_p(_chk(images, torch.uint8)), _p(out), B, H, W, 1 if dtype == F32 else 0, _s())
    return out


def vae_posterior(moments, qw, qb, scaling_factor, eps=None, want_moments=False):
    """The tail of AutoencoderKL.encode in one launch (sidlsg_vae_posterior).  moments: [B, h, w, 8] fp32 (the encoder's conv_out, NHWC);
    qw [8, 8] / qb [8] fp32: quant_conv; eps: [B, 4, h, w] fp32 or None (the mode).  -> z = (mean + std * eps) * scaling_factor fp32
    [B, 4, h, w], or (z, mean, logvar) with want_moments (logvar clamped to [-30, 20])."""
    if moments.dim() != 4 or moments.shape[3] != 8 or tuple(qw.shape) != (8, 8) or tuple(qb.shape) != (8,):
        raise RuntimeError(f'vae_posterior: moments {tuple(moments.shape)}, quant_conv {tuple(qw.shape)} / {tuple(qb.shape)}: expected [B, h, w, 8], [8, 8], [8]')
    B, h, w, _ = moments.shape
    if eps is not None and tuple(eps.shape) != (B, 4, h, w):
        raise RuntimeError(f'vae_posterior: eps {tuple(eps.shape)}: expected {(B, 4, h, w)}')
    z = torch.empty((B, 4, h, w), device=moments.device, dtype=F32)
    mean, logvar = (torch.empty_like(z), torch.empty_like(z)) if want_moments else (None, None)
    lib.sidlsg_vae_posterior(_p(_chk(moments, F32)), _p(_chk(qw, F32)), _p(_chk(qb, F32)), _p(_chk(eps, F32)) if eps is not None else None, _p(z),
                             _p(mean), _p(logvar), B, h * w, float(scaling_factor), _s())
    return (z, mean, logvar) if want_moments else z


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)      # the OpenAI constants the reference wrapper normalises with (networks/clip.py:26)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_patch_width(patch):
    """Kp: 3 * patch^2 rounded up to the multiple of 8 the GEMMs take as K (588 -> 592 for patch 14)."""
    return (3 * patch * patch + 7) // 8 * 8


def clip_patches(images_u8, size, patch, dtype=BF16, mean=CLIP_MEAN, std=CLIP_STD):
    """uint8 NCHW [B, 3, H, W] -> [B * (1 + (size / patch)^2), Kp] `dtype`: x / 255, bicubic resampling to size x size
    (F.interpolate(mode='bicubic', align_corners=False)), (v - mean) / std, unfolded into patch rows in (c, py, px) column order
    with a zero class-token row in front of every image and zero pad columns (sidlsg_clip_patches_u8): the A operand of the
    patch-embedding GEMM (networks/clip.py:33-37 in one launch)."""
    if images_u8.dim() != 4 or images_u8.shape[1] != 3:
        raise RuntimeError(f'clip_patches: expected uint8 [B, 3, H, W] images, got {tuple(images_u8.shape)}')
    if dtype not in (BF16, F32):
        raise RuntimeError(f'clip_patches: output dtype {dtype}: expected bf16 or fp32')
    if size % patch:
        raise RuntimeError(f'clip_patches: image size {size} is not a multiple of the patch size {patch}')
    B, _, H, W = images_u8.shape
    kp = clip_patch_width(patch)
    out = torch.empty((B * (1 + (size // patch) ** 2), kp), device=images_u8.device, dtype=dtype)
    _fn('clip_patches_u8', dtype)(_p(_chk(images_u8, torch.uint8)), _p(out), B, H, W, int(size), int(patch), kp, *(float(m) for m in mean),
                                  *(float(s) for s in std), _s())
    return out


_PIL_PLANS = {}
PIL_LDS_LIMIT = 64 * 1024          # sidlsg_pil_patches_u8: 3072 + 3 * band_rows * roundup(size, 4) bytes of LDS per workgroup


def _pil_plan(H, W, size, patch, device):
    """The coefficient banks of metrics.pil_crop_plan on `device`, built once per (source size, target, patch, device)."""
    key = (H, W, size, patch, str(device))
    if key not in _PIL_PLANS:
        from .metrics import pil_crop_plan
        plan = pil_crop_plan(H, W, size, patch)
        t = {k: torch.from_numpy(plan[k]).to(device) for k in ('hbounds', 'hcoef', 'vbounds', 'vcoef')}
        _PIL_PLANS[key] = (t, plan['hcoef'].shape[1], plan['vcoef'].shape[1], plan['band_rows'])
    return _PIL_PLANS[key]


def pil_patches(images_u8, size, patch, dtype=BF16, mean=CLIP_MEAN, std=CLIP_STD):
    """uint8 NCHW [B, 3, H, W] -> [B * (1 + (size / patch)^2), Kp] `dtype`, the layout of clip_patches, through open_clip's
    validation transform instead of the float interpolation: Pillow's 8-bit BICUBIC resize of the shorter side to `size` (antialiased,
    22-bit fixed point, two passes each rounded to 8 bits), centre crop, x / 255, (v - mean) / std (sidlsg_pil_patches_u8: one launch;
    bit-equal to PIL + torchvision's ToTensor / Normalize).  What HPSv2's `preprocess_val` feeds its ViT-H/14."""
    if images_u8.dim() != 4 or images_u8.shape[1] != 3:
        raise RuntimeError(f'pil_patches: expected uint8 [B, 3, H, W] images, got {tuple(images_u8.shape)}')
    if dtype not in (BF16, F32):
        raise RuntimeError(f'pil_patches: output dtype {dtype}: expected bf16 or fp32')
    if size % patch:
        raise RuntimeError(f'pil_patches: image size {size} is not a multiple of the patch size {patch}')
    B, _, H, W = images_u8.shape
    t, hk, vk, band_rows = _pil_plan(H, W, int(size), int(patch), images_u8.device)
    if 3072 + 3 * band_rows * ((size + 3) // 4 * 4) > PIL_LDS_LIMIT:
        raise RuntimeError(f'pil_patches: {H} x {W} -> {size}: a band of {patch} output rows reads {band_rows} source rows, more than the '
                           f'{PIL_LDS_LIMIT} bytes of LDS a workgroup stages them in')
    kp = clip_patch_width(patch)
    out = torch.empty((B * (1 + (size // patch) ** 2), kp), device=images_u8.device, dtype=dtype)
    _fn('pil_patches_u8', dtype)(_p(_chk(images_u8, torch.uint8)), _p(out), B, H, W, int(size), int(patch), kp, _p(t['hbounds']), _p(t['hcoef']),
                                 hk, _p(t['vbounds']), _p(t['vcoef']), vk, band_rows, *(float(m) for m in mean), *(float(s) for s in std), _s())
    return out


def gelu(x, mode):
    """MLP activation of a CLIP layer (sidlsg_gelu): mode 'quick_gelu' = x * sigmoid(1.702 x), 'gelu' = the exact erf GELU."""
    if mode not in ('quick_gelu', 'gelu'):
        raise ValueError(f"gelu: mode {mode!r}: expected 'quick_gelu' or 'gelu'")
    _chk(x, ACT)
    y = torch.empty_like(x)
    if x.numel():
        _fn('gelu', x.dtype)(_p(x), _p(y), x.numel(), 0 if mode == 'quick_gelu' else 1, _s())
    return y


CAUSAL_MAX_TOKENS = 128            # sidlsg_attn_causal_fwd: the whole sequence of a head lives in one workgroup
CAUSAL_MAX_HEAD_DIM = 128


def causal_attention(q, k, v, heads):
    """softmax(mask(q k^T / sqrt(D))) v per head, key j visible to query i iff j <= i (sidlsg_attn_causal_fwd): q, k, v [B, N, heads * D]
    bf16 or fp32 of one shape with unit channel stride -- contiguous, or column slices of a wider buffer (a fused q|k|v projection,
    consumed in place).  1 <= N <= 128, D a multiple of 8 up to 128.  Forward only; -> [B, N, heads * D]."""
    for t in (q, k, v):
        if not t.is_cuda:
            raise RuntimeError('sid_lsg_amd ops need CUDA(HIP) tensors: there is no CPU fallback')
        if t.requires_grad:
            raise RuntimeError('causal_attention is forward only (the text encoder is frozen): got a tensor that requires grad')
        if t.dtype not in (BF16, F32) or t.dtype != q.dtype or t.dim() != 3 or t.shape != q.shape or t.stride(2) != 1:
            raise RuntimeError(f'causal_attention: expected three bf16 or fp32 [B, N, C] tensors of one shape and dtype with unit channel '
                               f'stride, got {tuple(t.shape)} {t.dtype}')
    B, N, C = q.shape
    if heads <= 0 or C % heads or B == 0:
        raise RuntimeError(f'causal_attention: {C} channels do not split into {heads} heads (batch {B})')
    D = C // heads
    if not 1 <= N <= CAUSAL_MAX_TOKENS or D % 8 or D > CAUSAL_MAX_HEAD_DIM:
        raise RuntimeError(f'causal_attention: N = {N}, head dim {D}: the kernel takes 1 <= N <= {CAUSAL_MAX_TOKENS} and a head dim that '
                           f'is a multiple of 8 up to {CAUSAL_MAX_HEAD_DIM}')
    o = torch.empty((B, N, C), device=q.device, dtype=q.dtype)
    _fn('attn_causal_fwd', q.dtype)(_p(q), _p(k), _p(v), _p(o), B, heads, N, D, q.stride(1), k.stride(1), v.stride(1), C, q.stride(0),
                                    k.stride(0), v.stride(0), N * C, _s())
    return o


def causal_self_attention(qkv, heads):
    """qkv: [B, N, 3C] (the fused q|k|v projection of a CLIP text layer, read in place) -> [B, N, C]; forward only."""
    if qkv.dim() != 3 or qkv.shape[2] % 3:
        raise RuntimeError(f'causal_self_attention: expected a [B, N, 3C] tensor, got {tuple(qkv.shape)}')
    C = qkv.shape[2] // 3
    return causal_attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], heads)


def text_embed(ids, tok, pos, dtype=BF16):
    """int64 token ids [B, L] -> [B * L, D] `dtype`: tok[ids] + pos[:L], summed in fp32 and rounded once (sidlsg_text_embed).  tok [V, D]
    and pos [P >= L, D] are fp32 on the GPU.  Host ids are checked here (ValueError naming the id) and copied; for device ids the
    kernel writes the row of an id outside [0, V) as NaN and reads nothing for it."""
    _chk(tok, F32)
    _chk(pos, F32)
    if dtype not in (BF16, F32):
        raise RuntimeError(f'text_embed: output dtype {dtype}: expected bf16 or fp32')
    if ids.dim() != 2 or ids.dtype != torch.int64 or 0 in ids.shape:
        raise RuntimeError(f'text_embed: expected non-empty int64 [B, L] token ids, got {tuple(ids.shape)} {ids.dtype}')
    if tok.dim() != 2 or pos.dim() != 2 or tok.shape[1] != pos.shape[1] or tok.shape[1] % 8:
        raise RuntimeError(f'text_embed: tables {tuple(tok.shape)} and {tuple(pos.shape)}: expected [V, D] and [P, D], D a multiple of 8')
    B, L = ids.shape
    V, D = tok.shape
    if L > pos.shape[0]:
        raise RuntimeError(f'text_embed: {L} tokens per row, but only {pos.shape[0]} position embeddings')
    if not ids.is_cuda:
        bad = ids[(ids < 0) | (ids >= V)]
        if bad.numel():
            raise ValueError(f'text_embed: token id {int(bad[0])} is outside the vocabulary [0, {V})')
        ids = ids.to(tok.device)
    ids = ids.contiguous()
    out = torch.empty((B * L, D), device=tok.device, dtype=dtype)
    _fn('text_embed', dtype)(_p(ids), _p(tok), _p(pos), _p(out), B, L, D, V, pos.shape[0], _s())
    return out


def clip_score(image_embeds, text_embeds):
    """[B, F] image and text embeddings (both bf16 or both fp32) -> ([B, 2F] fp32 = F.normalize(image) | F.normalize(text), the
    reference wrapper's return value, and [B] fp32 cosines) (sidlsg_clip_score)."""
    _chk(image_embeds, ACT)
    _chk(text_embeds, image_embeds.dtype)
    if image_embeds.dim() != 2 or image_embeds.shape != text_embeds.shape or 0 in image_embeds.shape:
        raise RuntimeError(f'clip_score: image {tuple(image_embeds.shape)} and text {tuple(text_embeds.shape)}: expected two equal non-empty [B, F]')
    B, F = image_embeds.shape
    feats = torch.empty((B, 2 * F), device=image_embeds.device, dtype=F32)
    cosine = torch.empty(B, device=image_embeds.device, dtype=F32)
    lib.sidlsg_clip_score(_p(image_embeds), _p(text_embeds), 1 if image_embeds.dtype == F32 else 0, _p(feats), _p(cosine), B, F, _s())
    return feats, cosine


F16 = torch.float16


def _pr_features(x, name):
    """A feature matrix for the precision / recall kernels: fp16 [n, F] on the device, F padded with zero columns to a multiple of
    32 (zeros change neither a norm nor a dot product)."""
    if x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise RuntimeError(f'{name}: expected a non-empty [n, F] feature matrix, got {tuple(x.shape)}')
    _chk(x, F16)
    pad = -x.shape[1] % 32
    return torch.nn.functional.pad(x, [0, pad]) if pad else x


def pr_distances(rows, cols):
    """[R, C] fp16 distances between fp16 feature sets (sidlsg_pr_distances): the dense form of the precision / recall kernels,
    the reference's `compute_distances` (metrics/sid_precision_recall.py:19-32) without its host round trip."""
    rows, cols = _pr_features(rows, 'pr_distances'), _pr_features(cols, 'pr_distances')
    if rows.shape[1] != cols.shape[1]:
        raise RuntimeError(f'pr_distances: feature widths differ ({rows.shape[1]} vs {cols.shape[1]})')
    out = torch.empty((rows.shape[0], cols.shape[0]), device=rows.device, dtype=F16)
    lib.sidlsg_pr_distances(_p(rows), rows.shape[0], _p(cols), cols.shape[0], rows.shape[1], _p(out), _s())
    return out


PR_MAX_FUSED_K = 7


def pr_kth_radius(manifold, k):
    """[N] fp16: per row of `manifold` the (k+1)-th smallest distance to the rows of the same set, itself included
    (`dist.kthvalue(k + 1)`, :59).  k <= 7 runs fused (sidlsg_pr_kth_radius, no [N, N] matrix); a larger k goes through the
    dense kernel in row blocks and torch.kthvalue on the device -- the same distances, bit for bit."""
    manifold = _pr_features(manifold, 'pr_kth_radius')
    n = manifold.shape[0]
    if not 0 <= k < n:
        raise RuntimeError(f'pr_kth_radius: k = {k} needs a set of at least k + 1 rows, got {n}')
    if k > PR_MAX_FUSED_K:
        return torch.cat([pr_distances(blk, manifold).float().kthvalue(k + 1).values.to(F16) for blk in manifold.split(8192)])
    out = torch.empty(n, device=manifold.device, dtype=F16)
    lib.sidlsg_pr_kth_radius(_p(manifold), n, manifold.shape[1], int(k), _p(out), _s())
    return out


def pr_member(probes, manifold, radius):
    """[P] bool: probe i lies inside the manifold, i.e. within radius[j] of some manifold row j (sidlsg_pr_member; :64)."""
    probes, manifold = _pr_features(probes, 'pr_member'), _pr_features(manifold, 'pr_member')
    if probes.shape[1] != manifold.shape[1] or radius.shape != (manifold.shape[0],):
        raise RuntimeError(f'pr_member: probes {tuple(probes.shape)}, manifold {tuple(manifold.shape)}, radius {tuple(radius.shape)}')
    out = torch.empty(probes.shape[0], device=probes.device, dtype=torch.uint8)
    lib.sidlsg_pr_member(_p(probes), probes.shape[0], _p(manifold), manifold.shape[0], probes.shape[1], _p(_chk(radius, F16)), _p(out), _s())
    return out.bool()


PAIR_KERNEL_POLY3, PAIR_KERNEL_RBF = 0, 1


def pair_kernel_sums(x, y, kind, p0, p1=0.0, idx_x=None, idx_y=None):
    """[S, 5] fp64 = (Sxx, Syy, Sxy, Txx, Tyy) per subset (sidlsg_pair_kernel_sums): the sums over all ordered pairs of rows, the
    diagonal included (S), and over the pairs i == j of the symmetric passes (T), of
        kind 0:  (p0 g + p1)^3                      g = a . b as an fp32 fma chain on the f32 MFMA
        kind 1:  1 - exp(-p0 |a - b|^2)             the complement of the RBF kernel value
    summed in fp64 in a fixed order.  x [nx, F], y [ny, F] fp32 (x may be y).  idx_x [S, mx], idx_y [S, my] int32: subset s uses the
    rows x[idx_x[s]] and y[idx_y[s]] (both or neither; neither = every row in order, S = 1).  No [n, n] matrix and no gathered
    copy is formed.  F is padded with zero columns to a multiple of 4 (zeros change neither a norm nor a dot product)."""
    for t, name in ((x, 'x'), (y, 'y')):
        _chk(t, F32)
        if t.dim() != 2 or t.shape[0] == 0 or t.shape[1] == 0:
            raise RuntimeError(f'pair_kernel_sums: {name}: expected a non-empty [n, F] feature matrix, got {tuple(t.shape)}')
    if x.shape[1] != y.shape[1] or x.device != y.device:
        raise RuntimeError(f'pair_kernel_sums: x {tuple(x.shape)} on {x.device} and y {tuple(y.shape)} on {y.device}: one feature width, one device')
    if kind not in (PAIR_KERNEL_POLY3, PAIR_KERNEL_RBF):
        raise RuntimeError(f'pair_kernel_sums: kind {kind!r}: expected 0 (polynomial) or 1 (RBF)')
    if (idx_x is None) != (idx_y is None):
        raise RuntimeError('pair_kernel_sums: index lists are given for both sides or for neither')
    same = y is x
    pad = -x.shape[1] % 4
    if pad:
        x = torch.nn.functional.pad(x, [0, pad])
        y = x if same else torch.nn.functional.pad(y, [0, pad])
    x = x.contiguous()
    y = x if same else y.contiguous()
    S, mx, my = 1, x.shape[0], y.shape[0]
    if idx_x is not None:
        for t, n, name in ((idx_x, x.shape[0], 'idx_x'), (idx_y, y.shape[0], 'idx_y')):
            _chk(t, torch.int32)
            if t.dim() != 2 or t.device != x.device:
                raise RuntimeError(f'pair_kernel_sums: {name}: expected int32 [S, m] on {x.device}, got {tuple(t.shape)} on {t.device}')
            if t.numel() and not bool(((t >= 0) & (t < n)).all()):
                raise RuntimeError(f'pair_kernel_sums: {name} addresses rows outside 0 .. {n - 1}')
        if idx_x.shape[0] != idx_y.shape[0]:
            raise RuntimeError(f'pair_kernel_sums: {idx_x.shape[0]} subsets of x and {idx_y.shape[0]} of y')
        idx_x, idx_y = idx_x.contiguous(), idx_y.contiguous()
        S, mx, my = idx_x.shape[0], idx_x.shape[1], idx_y.shape[1]
    nws = lib.sidlsg_pair_kernel_sums_ws_doubles.raw(S, mx, my)
    if nws < 0:
        raise RuntimeError(f'pair_kernel_sums: {S} subsets of {mx} x {my} rows: need 1 <= S <= 65535, 1 <= m <= 2^24 and a workspace below 2^31 doubles')
    ws = torch.empty(nws, device=x.device, dtype=torch.float64)
    out = torch.empty((S, 5), device=x.device, dtype=torch.float64)
    lib.sidlsg_pair_kernel_sums(_p(x), x.shape[0], _p(y), y.shape[0], x.shape[1], _p(idx_x), _p(idx_y), S, mx, my, int(kind), float(p0), float(p1),
                                _p(out), _p(ws), _s())
    return out


# ---- FID Inception-v3 detector (csrc/inception.hip): fp32 NHWC, forward only ----
POOL_MAX, POOL_MEAN = 0, 1


def _slice_out(name, out, shape, col, width, device):
    """The [B, Ho, Wo, ld] fp32 buffer a launch writes columns col .. col + width - 1 of (a fresh [.., width] one when out is None)."""
    if out is None:
        if col:
            raise RuntimeError(f'{name}: a column offset needs the buffer it counts in')
        return torch.empty(shape + (width,), device=device, dtype=F32)
    _chk(out, F32)
    if out.dim() != 4 or tuple(out.shape[:3]) != shape or col < 0 or col % 4 or col + width > out.shape[3]:
        raise RuntimeError(f'{name}: output {tuple(out.shape)} does not hold columns {col} .. {col + width - 1} of a {shape} image')
    return out


def conv2d_relu_f32(x, w, bias, stride=1, padding=(0, 0), relu=True, out=None, col=0):
    """act(conv2d(x, w) + bias) (sidlsg_conv2d_relu_f32).  x [B, H, W, ldx] fp32 NHWC, of which the first Cin channels are read;
    w [Cout, KH, KW, Cin]; bias [Cout] (the folded BatchNorm shift).  -> [B, Ho, Wo, Cout], or columns col .. col + Cout - 1 of
    `out` [B, Ho, Wo, ldc]: a branch writes its slice of the block's output and the other columns keep their bits."""
    _chk(x, F32), _chk(w, F32), _chk(bias, F32)
    if x.dim() != 4 or w.dim() != 4 or x.shape[3] < w.shape[3] or bias.shape != (w.shape[0],):
        raise RuntimeError(f'conv2d_relu_f32: x {tuple(x.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}')
    B, H, W, ldx = x.shape
    Cout, KH, KW, Cin = w.shape
    ph, pw = padding
    Ho, Wo = (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1
    if Ho < 1 or Wo < 1:
        raise RuntimeError(f'conv2d_relu_f32: a {KH} x {KW} kernel does not fit a {H} x {W} image with padding {padding}')
    out = _slice_out('conv2d_relu_f32', out, (B, Ho, Wo), col, Cout, x.device)
    lib.sidlsg_conv2d_relu_f32(_p(x), ldx, _p(w), out.data_ptr() + 4 * col, out.shape[3], _p(bias), B, H, W, Cin, Cout, KH, KW, stride, ph, pw,
                               1 if relu else 0, _s())
    return out


def pool2d_f32(x, k, stride, pad=0, mode=POOL_MAX, out=None, col=0):
    """k x k pooling of x [B, H, W, C] fp32 NHWC (sidlsg_pool2d_f32): POOL_MAX (the bits of F.max_pool2d) or POOL_MEAN over the taps
    inside the image (count_include_pad=False).  -> [B, Ho, Wo, C], or columns col .. col + C - 1 of `out` [B, Ho, Wo, ldy]."""
    _chk(x, F32)
    if x.dim() != 4:
        raise RuntimeError(f'pool2d_f32: x {tuple(x.shape)}: expected [B, H, W, C]')
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if Ho < 1 or Wo < 1:
        raise RuntimeError(f'pool2d_f32: a {k} x {k} window does not fit a {H} x {W} image with padding {pad}')
    out = _slice_out('pool2d_f32', out, (B, Ho, Wo), col, C, x.device)
    lib.sidlsg_pool2d_f32(_p(x), C, out.data_ptr() + 4 * col, out.shape[3], B, H, W, C, k, stride, pad, int(mode), _s())
    return out


def inception_input_u8(images, out=None):
    """uint8 NCHW [B, 3, H, W] -> [B, 299, 299, 4] fp32 NHWC (sidlsg_inception_input_u8): the detector's legacy-TF bilinear resize and
    (v - 128) / 128 in one launch; channel 3 is zero (the stem convolution has zero weights there)."""
    _chk(images, torch.uint8)
    if images.dim() != 4 or images.shape[1] != 3:
        raise RuntimeError(f'inception_input_u8: expected uint8 [B, 3, H, W], got {tuple(images.shape)}')
    B, _, H, W = images.shape
    if out is None:
        out = torch.empty((B, 299, 299, 4), device=images.device, dtype=F32)
    elif _chk(out, F32).shape != (B, 299, 299, 4):
        raise RuntimeError(f'inception_input_u8: output {tuple(out.shape)} for {B} images')
    lib.sidlsg_inception_input_u8(_p(images), _p(out), B, H, W, _s())
    return out


def _det_synced(backward):
    @functools.wraps(backward)
    def wrapper(*args):
        sync_deterministic()
        return backward(*args)
    return staticmethod(wrapper)


# every backward of this module sees the current deterministic mode (see sync_deterministic)
for _cls in list(globals().values()):
    if isinstance(_cls, type) and issubclass(_cls, torch.autograd.Function) and _cls.__module__ == __name__ and 'backward' in _cls.__dict__:
        _cls.backward = _det_synced(_cls.__dict__['backward'].__func__)
del _cls
