"""tests/gemm_cases.py checked on the CPU: its references against F.conv2d / matmul / autograd in fp64, every case below 2^24 and with
enough bf16 rounding to notice a wrong rounding mode (the e4m3 rows: every operand an e4m3 value, every scaled sum below 2^24), its oracle
against planted mutants of a correct result (a dropped K chunk, swapped taps, a wrong image's row; for the e4m3 kernels the scale of another
channel, a wrong halo bit, a part-filled channel chunk that is not zeroed, a dropped split-K slab), and -- in a child process
that sees no GPU -- the dispatch record of every table row against the kernel the row names."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc      # noqa: E402

BF16, F32, F64, F8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
FWD = gc.GEMM_CASES + gc.CONV_CASES
FP8_CONV = tuple(c for c in gc.FP8_CASES if c['ep'] == 'conv')
ids = lambda cases: [c['id'] for c in cases]      # noqa: E731


# ---- references ----------------------------------------------------------------------------------------------------------------------
def torch_conv(c, x, w):
    """F.conv2d in fp64 on the NCHW view of a case's operands -> [M, N]."""
    Cin, Cout = c['Cin'], c['Cout']
    xi = x.float().to(F64).permute(0, 3, 1, 2)
    if c['ups']:
        xi = F.interpolate(xi, scale_factor=2, mode='nearest')
    wt = w.float().to(F64).view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    if c['ep'] == 'conv_br':
        y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), wt, stride=2)
    else:
        y = F.conv2d(xi, wt, stride=c['stride'], padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, Cout)


@pytest.mark.parametrize('c', gc.CONV_CASES + FP8_CONV, ids=ids(gc.CONV_CASES + FP8_CONV))
def test_conv_reference_is_conv2d(c):
    o = gc.fwd_operands(c)
    assert torch.equal(gc.contract(c, o['a'], o['w']), torch_conv(c, o['a'], o['w']))


@pytest.mark.parametrize('c', [c for c in gc.WGRAD_CASES if c['ep'] == 'wgrad_conv'], ids=lambda c: c['id'])
def test_conv_wgrad_reference_is_autograd(c):
    o = gc.wgrad_operands(c)
    w = torch.zeros(c['Cout'], 9 * c['Cin'], dtype=F64, requires_grad=True)
    (torch_conv(c, o['a'], w) * o['dy'].to(F64)).sum().backward()
    dw, db = gc.wgrad_reference(c, o)
    assert torch.equal(dw, w.grad) and torch.equal(db, o['dy'].to(F64).sum(0))
    assert dw.abs().max() + 1000 < 2 ** 24


@pytest.mark.parametrize('stride,ups', [(1, 0), (2, 0), (1, 1)])
@pytest.mark.parametrize('hw', [(6, 10), (9, 7)])
def test_dgrad_chain_is_the_conv_gradient(stride, ups, hw):
    """The zero-insert -> conv and conv -> sum-pool chains equal autograd's data gradient; on these operands both bf16 rounding points are exact
    where the values stay below 256, so the chain is compared before rounding through a weight of one tap pattern that keeps them small."""
    Hs, Ws = hw
    if ups and (Hs % 2 or Ws % 2):
        Hs, Ws = Hs + 1, Ws + 1
    B, Cin, Cout = 2, 8, 16
    g = torch.Generator().manual_seed(5)
    c = dict(ep='conv', Cin=Cin, Cout=Cout, stride=stride, ups=ups)
    w = gc.ints(g, (Cout, 9 * Cin), -1, 1, BF16)
    x = torch.zeros(B, Hs, Ws, Cin, dtype=F64, requires_grad=True)
    y = torch_conv(c, x, w)
    H, W = (2 * Hs, 2 * Ws) if ups else (Hs, Ws)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = gc.ints(g, (B, Ho, Wo, Cout), -1, 1, BF16)
    (y * dy.to(F64).reshape(-1, Cout)).sum().backward()
    assert x.grad.abs().max() <= 256          # every integer up to 256 is a bf16 value: no rounding point can hide a difference
    assert torch.equal(gc.dgrad_reference(dy, w, (B, Hs, Ws, Cin), stride, ups).to(F64), x.grad)


# ---- every case: exact in fp32 whatever the order, and rounding that matters -----------------------------------------------------------
def _abs_bound(c, o):
    """No partial sum of any order exceeds sum_k |a_k| |w_k| <= 3 * 2 * K."""
    assert o['a'].abs().max() <= 3 and o['w'].abs().max() <= 2 and (not c['g2'] or o['w1'].abs().max() <= 2)
    return 6 * gc.mnk(c)[2]


@pytest.mark.parametrize('c', FWD, ids=ids(FWD))
def test_forward_case_is_exact_and_rounds(c):
    o = gc.fwd_operands(c)
    bound = _abs_bound(c, o)
    assert 2 * bound + 4000 < 2 ** 24, bound        # alpha <= 2; bias + row vector + residual + previous contents < 4000
    M, N, K = gc.mnk(c)
    if c['ep'] == 'gemm':      # fp32 matmul of these operands IS the fp64 product
        assert torch.equal((o['a'].float() @ o['w'].float().t()).double(), gc.contract(c, o['a'], o['w']))
    for feat, rpb in gc.fwd_runs(c):
        f = gc.FEATS[feat]
        _, x = gc.fwd_reference(c, feat, rpb)
        assert x.shape == (M, N)
        if f.get('silu'):
            continue
        gc.round_out(x, F32)                        # asserts exactness in fp32
        if not f.get('f32') and f.get('bias'):      # a bf16 output with bias / residual magnitudes of ~1000 (without them |x| < 256 at short K: nothing to round)
            frac = gc.needs_rounding(x).double().mean().item()
            tie = gc.is_tie(x)
            assert frac >= 0.10 and tie.any(), f'{c["id"]} {feat}: {frac:.3f} of the outputs need rounding, {int(tie.sum())} ties'
            if N * M >= 1000:
                up = gc.tie_goes_up(x)
                assert (tie & up).any() and (tie & ~up).any(), 'ties must go both ways (to even)'


def _abs_sum(c, a, w):
    """max over the outputs of sum_k |a_k| |w_k| (a as the loader converts it): no partial sum of any order exceeds it."""
    return gc.contract(c, a.float().abs().to(a.dtype), w.float().abs().to(w.dtype)).max().item()


@pytest.mark.parametrize('c', gc.FP8_CASES, ids=ids(gc.FP8_CASES))
def test_fp8_case_is_exact_and_rounds(c):
    o = gc.fwd_operands(c)
    M, N, K = gc.mnk(c)
    mx8 = c['fp8'] == 'mx8'
    assert o['w'].dtype == F8 and o['a'].dtype == (F8 if mx8 else BF16)
    # every operand is what its bytes say: integers that survive the e4m3 round trip unchanged (the fp8w activations as the loader converts them)
    a = o['a'].float()
    if c['sat']:
        big = a.abs() >= 448
        assert 0.003 < big.float().mean().item() < 0.03 and (a.abs() > 448).any(), 'the sat row needs entries at and past +-448'
        assert set(a[big].clamp(-448, 448).tolist()) == {448.0, -448.0}
        a = a.clamp(-448, 448)
        small = a[~big]
    else:
        small = a
    assert small.abs().max() <= 3 and torch.equal(small, small.round())
    assert torch.equal(a.to(F8).float(), a)
    for k in ('w', 'w1') if c['g2'] else ('w',):
        wf = o[k].float()
        assert wf.abs().max() <= 2 and torch.equal(wf, wf.round()) and torch.equal(wf.to(F8).float(), wf)
    # the scales: exactly representable with two significant bits, a period that divides no tile, fragment or wave width
    for vals in (gc.WSCALES, gc.WSCALES1):
        assert all(len(vals) % d and d % len(vals) for d in (4, 8, 16, 80)) and all(v * 4 == int(v * 4) and v in (0.25, 0.5, 1, 2, 3, 4, 6) for v in vals)
    assert torch.equal(o['wscale'], gc.wscale_of(N, gc.WSCALES)) and (not c['g2'] or torch.equal(o['wscale1'], gc.wscale_of(N, gc.WSCALES1)))
    for d in (4, 8, 16, 80):
        if N > d:
            assert not torch.equal(o['wscale'][d:], o['wscale'][:-d]), f'a scale read {d} channels off would go unnoticed'
    bound = max(_abs_sum(c, o['a'], o[k]) for k in (('w', 'w1') if c['g2'] else ('w',)))
    assert bound * max(gc.WSCALES + gc.WSCALES1) * 2 + 4000 < 2 ** 24, bound      # alpha <= 2; bias + row vector + residual + previous contents < 4000
    if c['small_ws']:
        assert 2 * M * N * 4 > gc.MX8_SMALL_WS_BYTES
    for feat, rpb in gc.fwd_runs(c):
        f = gc.FEATS[feat]
        _, x = gc.fwd_reference(c, feat, rpb)
        assert x.shape == (M, N)
        if f.get('silu'):
            continue
        gc.round_out(x, F32)                        # asserts exactness in fp32
        if not f.get('f32') and f.get('bias'):
            frac = gc.needs_rounding(x).double().mean().item()
            tie = gc.is_tie(x)
            assert frac >= 0.10 and tie.any(), f'{c["id"]} {feat}: {frac:.3f} of the outputs need rounding, {int(tie.sum())} ties'
            if N * M >= 1000:
                up = gc.tie_goes_up(x)
                assert (tie & up).any() and (tie & ~up).any(), 'ties must go both ways (to even)'


def test_fp8_rows_cover_both_epilogues_split_and_unsplit():
    """bf16 outputs leave gemm_mx8_kernel through its LDS ring, fp32 / accumulating ones through the direct epilogue: both on split and unsplit rows."""
    for split in (False, True):
        rows = [c for c in gc.MX8_CASES if (c['expect']['splits'] > 1) == split]
        for ep in ('gemm', 'conv'):
            assert any(c['ep'] == ep and {'plain', 'all', 'f32', 'accum'} <= set(c['feats']) for c in rows), (split, ep)
    assert all(set(c['feats']) == set(gc.ALL_FEATS) for c in gc.FP8_CASES)


@pytest.mark.parametrize('c', gc.WGRAD_CASES, ids=ids(gc.WGRAD_CASES))
def test_wgrad_case_is_exact(c):
    o = gc.wgrad_operands(c)
    M, N, K = gc.mnk(c)
    dw, db = gc.wgrad_reference(c, o)
    assert dw.shape == (N, K) and db.shape == (N,)
    assert 9 * M + 1000 < 2 ** 24          # |dy| |a| <= 9 per row
    if c['ep'] == 'wgrad':
        assert torch.equal((o['dy'].float().t() @ o['a'].float()).double(), dw)
    if c['small_ws']:
        assert 2 * N * K * 4 > gc.SMALL_WS_BYTES


def test_weight_gradients_stay_exact_at_16384_rows():
    assert 9 * 16384 + 1000 < 2 ** 24


# ---- the oracle catches planted mutants -------------------------------------------------------------------------------------------------
def _case(cid):
    return next(c for c in gc.ALL_CASES if c['id'] == cid)


def test_mutant_last_k_chunk_dropped():
    c = _case('gemm-129x136x136')
    o, x = gc.fwd_reference(c, 'bias')
    want = gc.round_out(x, BF16)
    a = o['a'].clone()
    a[:, -8:] = 0
    bad = gc.round_out(gc.contract(c, a, o['w']) + o['bias'].double(), BF16)
    assert gc.exact_mismatch(want, want) == '' and gc.exact_mismatch(bad, want) != ''
    # one dropped K ELEMENT of one row, the error the old relative bar let through at K >= 320
    c = _case('gemm-130x12x320')
    o, x = gc.fwd_reference(c, 'bias')
    a = o['a'].clone()
    k = int((a[7] * o['w'][3]).abs().argmax())          # a product that is not zero
    a[7, k] = 0
    bad = gc.round_out(gc.contract(c, a, o['w']) + o['bias'].double(), F32)
    assert gc.exact_mismatch(bad, gc.round_out(x, F32)) != ''


def test_mutant_conv_taps_swapped():
    c = _case('conv-2x12x20x8-320')
    o, x = gc.fwd_reference(c, 'plain')
    w = o['w'].view(320, 9, 8).clone()
    w[:, [1, 3]] = w[:, [3, 1]]
    bad = gc.contract(c, o['a'], w.view(320, 72))
    assert gc.exact_mismatch(gc.round_out(bad, BF16), gc.round_out(x, BF16)) != ''


def test_mutant_row_from_the_neighbouring_image():
    """A tap that leaves the image at its last row must read zero, not the first row of the next image."""
    c = _case('conv-2x12x20x8-320')
    o, x = gc.fwd_reference(c, 'plain')
    xs = o['a'].double()
    wrapped = torch.cat([xs[0], xs[1][:1]], 0)[None]                      # image 0 with image 1's first row below it
    cc = dict(c, B=1, Hs=13)
    bad_last_row = gc.contract(cc, wrapped, o['w']).view(13, 20, 320)[11]
    bad = x.clone().view(2, 12, 20, 320)
    bad[0, 11] = bad_last_row
    msg = gc.exact_mismatch(gc.round_out(bad.view(-1, 320), BF16), gc.round_out(x, BF16))
    assert msg != '' and 'first at (2' in msg                             # rows 220 .. 239: the last image row of image 0


def test_mutant_rowvec_of_the_wrong_image():
    c = _case('conv-2x12x20x8-320')
    rpb = 240
    o, x = gc.fwd_reference(c, 'bias_rv', rpb)
    bad = x.clone()
    bad[192:240] += (o['rv'][rpb][1] - o['rv'][rpb][0]).double()          # the tail rows of the tile that spans both images take image 1's vector
    assert gc.exact_mismatch(gc.round_out(bad, BF16), gc.round_out(x, BF16)) != ''


def test_mutant_truncation_instead_of_rne():
    c = _case('gemm-129x136x136')
    _, x = gc.fwd_reference(c, 'bias_res')
    want = gc.round_out(x, BF16)
    bad = gc.truncate_bf16(x.to(F32))
    msg = gc.exact_mismatch(bad, want)
    assert msg != ''
    exact = ~gc.needs_rounding(x)
    assert torch.equal(gc.bits(bad)[exact], gc.bits(want)[exact])          # (the mutant is right wherever nothing needs rounding)


def _rejected(bad64, x64):
    """Both output types must tell the mutant from the result."""
    return all(gc.exact_mismatch(gc.round_out(bad64, t), gc.round_out(x64, t)) != '' for t in (BF16, F32))


def test_mutant_scale_of_channel_n_plus_4():
    for cid in ('mx8-130x160x16', 'fp8w-200x136x80', 'mx8conv-3x9x7x16-160'):
        c = _case(cid)
        o, x = gc.fwd_reference(c, 'bias')
        acc = gc.contract(c, o['a'], o['w'])
        assert torch.equal(acc * o['wscale'].double() + o['bias'].double(), x)
        for d in (4, 8, 16, 80):
            if d < c.get('N', c.get('Cout')):
                assert _rejected(acc * o['wscale'].roll(-d).double() + o['bias'].double(), x), (cid, d)


def test_mutant_halo_tap_dropped_at_an_image_corner():
    """One bit of gemm_mx8_kernel's 9-bit halo mask wrong for one pixel: the top-left pixel of the second image loses its right neighbour."""
    c = _case('mx8conv-2x12x20x48-160')
    o, x = gc.fwd_reference(c, 'plain')
    Cin, m = c['Cin'], 12 * 20                                               # row m: image 1, pixel (0, 0)
    tap = 1 * 3 + 2                                                          # (dh, dw) = (1, 2): input pixel (0, 1), inside the image
    lost = o['a'].float().double()[1, 0, 1] @ o['w'].float().double()[:, tap * Cin:(tap + 1) * Cin].t() * o['wscale'].double()
    assert (lost != 0).any()
    bad = x.clone()
    bad[m] -= lost
    assert _rejected(bad, x)
    # and the opposite error: a tap outside the image (its memory holds the last pixel of image 0) read instead of zero
    tap = 1 * 3 + 0
    extra = o['a'].float().double()[0, 11, 19] @ o['w'].float().double()[:, tap * Cin:(tap + 1) * Cin].t() * o['wscale'].double()
    bad = x.clone()
    bad[m] += extra
    assert (extra != 0).any() and _rejected(bad, x)


def test_mutant_partial_channel_chunk_meets_the_next_taps_weights():
    """Cin = 144 = 128 + 16: the second channel chunk of a tap holds 16 channels; the W tile's other 112 columns are the NEXT tap's weights of
    channels 0 .. 111.  The mutant lets the A lanes past Cin read on (into the next pixel's channels 0 .. 111) instead of zeros, for the centre tap."""
    for cid in ('mx8conv-1x10x6x144-320', 'mx8conv-1x10x6x144-320-smallws'):
        c = _case(cid)
        o, x = gc.fwd_reference(c, 'plain')
        Cin, M = c['Cin'], gc.mnk(c)[0]
        xf = torch.cat([o['a'].float().double().reshape(M, Cin), torch.zeros(1, Cin, dtype=F64)])
        extra = xf[1:, :112] @ o['w'].float().double()[:, 5 * Cin:5 * Cin + 112].t() * o['wscale'].double()
        assert _rejected(x + extra, x)


def test_mutant_last_splits_slab_dropped():
    c = _case('mx8-130x320x2064')
    assert c['expect']['splits'] == 4
    o, x = gc.fwd_reference(c, 'bias')
    a = o['a'].float()
    a[:, 3 * 5 * 128:] = 0                                                   # 17 K-tiles at 5 per split: the last split holds tiles 15 and 16
    bad = gc.contract(c, a.to(F8), o['w']) * o['wscale'].double() + o['bias'].double()
    assert _rejected(bad, x)
    a = o['a'].float()
    a[:, 2048:] = 0                                                          # only the ragged last chunk (16 bytes)
    assert _rejected(gc.contract(c, a.to(F8), o['w']) * o['wscale'].double() + o['bias'].double(), x)


@pytest.mark.parametrize('dtype', [BF16, F32])
def test_mutant_writes_outside_the_output(dtype):
    M, N, pad = 37, 24, 8
    fill = torch.zeros(M, N)
    for r, col in ((0, N), (M - 1, N), (M, 0), (M, N - 1), (M + gc.GUARD - 1, N + pad - 1), (5, N + pad - 1)):      # one past N; row M; the far corner
        whole, view = gc.guarded(M, N, pad, dtype, 'cpu', fill)
        assert gc.guard_damage(whole, M, N) == '' and view.stride(0) == N + pad
        whole[r, col] = 1.0
        assert f'row {r}, column {col}' in gc.guard_damage(whole, M, N)
    whole, view = gc.guarded(M, N, pad, dtype, 'cpu', fill)
    view[M - 1, N - 1] = 7.0                                                   # inside: not damage
    assert gc.guard_damage(whole, M, N) == ''
    whole, v = gc.poisoned_flat(torch.zeros(4, 6, dtype=F32), 'cpu')
    assert gc.flat_damage(whole, 24) == ''
    whole[24] = 0.0
    assert gc.flat_damage(whole, 24) != ''


def test_poisoned_inputs_are_nan_outside_the_logical_operand():
    t = gc.ints(torch.Generator().manual_seed(1), (5, 16), -3, 3, BF16)
    v = gc.poisoned(t, 8, 'cpu')
    assert v.stride(0) == 24 and torch.equal(v, t)
    whole = v._base if v._base is not None else v
    mask = torch.ones(whole.shape, dtype=torch.bool)
    mask[:5, :16] = False
    assert torch.isnan(whole.float()[mask]).all() and whole.shape == (5 + gc.GUARD, 24)


def test_rounding_predicates_agree_with_torch():
    x = torch.arange(-4100, 4100, dtype=F64) * 0.5
    r = gc.round_out(x, BF16).to(F64)
    assert torch.equal(gc.needs_rounding(x), r != x)
    lo = gc.truncate_bf16(x.to(F32)).to(F64)                 # the bf16 neighbour towards zero
    tie = gc.is_tie(x)
    assert tie.any() and torch.equal(tie, (x != lo) & ((x - lo).abs() * 2 == _ulp(lo)))
    assert torch.equal((r.abs() > x.abs())[tie], gc.tie_goes_up(x)[tie]) and gc.tie_goes_up(x)[tie].any() and not gc.tie_goes_up(x)[tie].all()


def _ulp(v64):
    """Spacing of the bf16 values at |v| (v a bf16 value, away from zero)."""
    b = gc.bits(v64.to(BF16))
    return ((b + 1).view(BF16).to(F64) - v64).abs()


def test_nan_in_the_output_is_reported():
    want = torch.zeros(3, 8, dtype=BF16)
    got = want.clone()
    got[1, 2] = float('nan')
    assert 'NaN' in gc.exact_mismatch(got, want)


# ---- which kernel each row reaches, checked without a GPU --------------------------------------------------------------------------------
def _worker():
    """Child process (no GPU visible): every call of every table row -> the dispatch record it left, as one JSON line.  Operands are
    addresses of a 16-byte-aligned host buffer (never dereferenced on the host); a fake workspace of the default size is registered."""
    assert os.environ.get('HIP_VISIBLE_DEVICES') == '-1'
    import ctypes
    from sid_lsg_amd._lib import lib
    lib.load()
    raw = ctypes.create_string_buffer(4096 + 16)
    ptr = (ctypes.addressof(raw) + 15) & ~15
    P = {k: ptr for k in ('a', 'w', 'w1', 'wscale', 'wscale1', 'c', 'bias', 'bias1', 'res', 'rv', 'dy', 'dw', 'db')}
    P['stream'] = None
    lib.sidlsg_set_workspace.raw(ptr, gc.WORKSPACE_BYTES)
    assert gc.last_launch(lib)['kernel'] == 'NONE'
    out = {}

    def call(name, args):
        before = gc.last_launch(lib)['seq']
        rc = getattr(lib, name).raw(*args)
        r = gc.last_launch(lib)
        assert rc != 0 and rc != -22, (name, rc)          # admitted, and HIP has no device: nothing ran
        assert r['seq'] == before + 1, (name, before, r)
        return r

    for c in gc.ALL_CASES:
        recs = []
        if c['ep'] in ('gemm', 'conv', 'conv_br'):
            old = lib.sidlsg_debug_set_p8.raw(c['p8'])
            if c['small_ws']:
                lib.sidlsg_set_workspace.raw(ptr, gc.MX8_SMALL_WS_BYTES)
            for feat, rpb in gc.fwd_runs(c):
                recs.append((f'{feat}/{rpb}', call(*gc.fwd_call(c, feat, rpb, P))))
            lib.sidlsg_set_workspace.raw(ptr, gc.WORKSPACE_BYTES)
            lib.sidlsg_debug_set_p8.raw(old)
        elif c['ep'] in ('wgrad', 'wgrad_conv'):
            if c['small_ws']:
                lib.sidlsg_set_workspace.raw(ptr, gc.SMALL_WS_BYTES)
            old = lib.sidlsg_set_deterministic.raw(1 if c['det'] else 0)
            for assign in (0, 1):
                recs.append((f'assign={assign}', call(*gc.wgrad_call(c, assign, P))))
            lib.sidlsg_set_deterministic.raw(old)
            lib.sidlsg_set_workspace.raw(ptr, gc.WORKSPACE_BYTES)
        else:
            jobs = gc.group_jobs(c, [(ptr,) * 4] * len(c['jobs']))
            recs.append(('group', call('sidlsg_wgrad_group160_bf16' if c['t160'] else 'sidlsg_wgrad_group_bf16', [ctypes.addressof(jobs), len(c['jobs']), None])))
        out[c['id']] = recs
    print('RESULT ' + json.dumps(out))


@pytest.fixture(scope='module')
def records():
    env = {k: v for k, v in os.environ.items() if not k.startswith('SIDLSG_') or k == 'SIDLSG_LIB'}      # the knobs at their defaults
    env.update(HIP_VISIBLE_DEVICES='-1', PYTHONPATH=gc.ROOT + os.pathsep + env.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=gc.ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def test_case_ids_are_unique():
    assert len({c['id'] for c in gc.ALL_CASES}) == len(gc.ALL_CASES)


@pytest.mark.parametrize('c', gc.ALL_CASES, ids=ids(gc.ALL_CASES))
def test_row_reaches_its_kernel(records, c):
    recs = records[c['id']]
    assert recs
    wrong = [m for m in (gc.record_mismatch(f"{c['id']} [{label}]", r, c['expect']) for label, r in recs) if m]
    assert not wrong, '\n'.join(wrong)


def test_every_kernel_id_is_in_the_table(records):
    seen = {r['kernel'] for recs in records.values() for _, r in recs}
    names = set(gc.kernel_ids().values())
    assert set(gc.UNREACHED) <= names and not (seen & set(gc.UNREACHED))
    assert names - seen == set(gc.UNREACHED), f'kernel ids without a table row: {sorted(names - seen - set(gc.UNREACHED))}'
    # every tile shape and MODE of gemm_bf16_kernel the dispatchers can choose, and both reductions of the weight gradients
    shapes = {(r['bm'], r['bn'], r['mode'], r['pad']) for recs in records.values() for _, r in recs if r['kernel'] == 'GEMM_BF16'}
    want = {(128, 64, 0, 1), (64, 64, 0, 1), (64, 128, 0, 1), (128, 128, 0, 1), (64, 160, 0, 1),
            (128, 64, 1, 1), (128, 64, 2, 1), (64, 64, 2, 1), (64, 128, 1, 1), (64, 128, 2, 1), (128, 128, 1, 1), (128, 128, 2, 1), (64, 160, 2, 1), (128, 160, 2, 1),
            (128, 128, 1, 0), (64, 64, 1, 0), (64, 64, 2, 0)}
    assert want <= shapes, sorted(want - shapes)
    parts = {(r['kernel'], r['partial']) for recs in records.values() for _, r in recs if r['kernel'].startswith('WGRAD')}
    assert {p for _, p in parts} == {'one', 'slabs', 'atomics'}


if __name__ == '__main__':
    _worker()
