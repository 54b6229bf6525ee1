"""IP-Adapter image prompts on the GPU: the two-set cross-attention kernel (csrc/ip_attn.hip) on the needle inputs of tests/ip_cases.py,
the adapter module (sid_lsg_amd.ip_adapter), HipUNet2DCondition.forward_nhwc(ip=...), the samplers and the command line against the fp64
torch.nn restatement of tests/ip_adapter_ref.py.  The HIP modules and the reference load one state dict through the published key
names.  tests/test_ip_cases_host.py asserts the preconditions: every wrong two-set attention misses the kernel bound tenfold, and the
seeded adapter changes the reference UNet's output by more than 10 %, so no tolerance below can be met by ignoring the state.

Every kernel call here goes through the layout the UNet uses: K | V fused in one [B, Nk, 2C] buffer, K2 | V2 a column slice at a non-zero
offset of a wide per-batch buffer whose other columns are NaN."""
import collections
import dataclasses
import glob
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import controlnet_ref as cr
import ip_adapter_ref as ir
import ip_cases as ic

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL = 1e-4      # max |err| / max |ref|: FP32_TOL of tests/test_gpu_controlnet.py
EINVAL = -22


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def close(got, ref, tol, name=''):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item() + 1e-30
    assert err <= tol * scale, f'{name}: max err {err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g} > {tol})'
    return err / scale


def rel_l2(got, ref):
    return float((got.detach().double().cpu() - ref.double()).norm() / ref.double().norm())


# ---- 1 - 3. the kernel ------------------------------------------------------------------------------------------------------------------
PAD = 8      # columns in front of and behind the K2 | V2 slice of the wide buffer


def device_operands(x, dev):
    """make_inputs' tensors as the UNet lays them out -> (q, kv [B, Nk, 2C], k2v2 view [B, Nk2, 2C] of a NaN-filled [B, Nk2, 2C + 16])."""
    q = x['q'].to(dev).contiguous()
    kv = torch.cat([x['k'], x['v']], -1).to(dev).contiguous()
    B, Nk2, C = x['k2'].shape
    wide = torch.full((B, Nk2, 2 * C + 2 * PAD), float('nan'), dtype=x['k2'].dtype, device=dev)
    view = wide[:, :, PAD:PAD + 2 * C]
    view.copy_(torch.cat([x['k2'], x['v2']], -1))
    return q, kv, view


def run_cross2(x, s, H, ps, dev):
    from sid_lsg_amd import ops
    q, kv, view = device_operands(x, dev)
    with torch.no_grad():
        return ops.cross_attention2(q, kv, view, H, s, prescaled=ps)


@pytest.mark.parametrize('ps', [False, True], ids=['plain', 'ps'])
@pytest.mark.parametrize('D', ic.GPU_WIDTHS)
def test_cross2_bf16_needles(dev, D, ps):
    """Both needle kinds at every shape, s = 1 and 0.5 alternating over the shapes, and the biased kind at Nk2 = 4 and 17: FWD_TOL per slice."""
    worst = 0.0
    for i, (nq, nk, nk2) in enumerate(ic.GPU_SHAPES):
        c = ic.Case2(2, 4, nq, nk, nk2, D, ps)
        kinds = ic.KINDS + (('biased',) if (nq, nk) == (130, 77) and nk2 in ic.GPU_BIASED_NK2 else ())
        for j, kind in enumerate(kinds):
            s = (1.0, 0.5)[(i + j) % 2]
            x = ic.case_inputs(c, kind)
            got = run_cross2(x, s, c.H, ps, dev)
            assert got.dtype == BF16
            worst = max(worst, ic.close_slices(got, ic.case_ref(c, kind, s), ic.FWD_TOL, c.H, f'{ic.case_id(c)} {kind} s={s}'))
    print(f'cross2 bf16 d{D}{" ps" if ps else ""}: worst per-slice error {worst:.5f} (bound {ic.FWD_TOL})')


@pytest.mark.parametrize('D', ic.GPU_WIDTHS + (4, 12, 100))
def test_cross2_f32_needles(dev, D):
    """The fp32 family on the same shapes (and three widths only it admits): 2e-5 per slice.  The one shape whose LDS image does not fit
    (128 + 4 keys at D = 160: 2 * 144 * 164 * 4 bytes) is refused by name."""
    from sid_lsg_amd import ops
    worst = 0.0
    for i, (nq, nk, nk2) in enumerate(ic.GPU_SHAPES):
        c = ic.Case2(2, 4, nq, nk, nk2, D, False)
        kinds = ic.KINDS + (('biased',) if (nq, nk) == (130, 77) and nk2 in ic.GPU_BIASED_NK2 else ())
        for j, kind in enumerate(kinds):
            s = (1.0, 0.5)[(i + j) % 2]
            x = ic.case_inputs(c, kind, F32)
            if 2 * ((nk + 15) // 16 * 16 + (nk2 + 15) // 16 * 16) * ((D + 15) // 16 * 16 + 4) * 4 > ops.CROSS2_LDS_BYTES:
                assert (nk, D) == (128, 160)
                with pytest.raises(RuntimeError, match='bytes of LDS'):
                    run_cross2(x, s, c.H, False, dev)
                continue
            got = run_cross2(x, s, c.H, False, dev)
            assert got.dtype == F32
            worst = max(worst, ic.close_slices(got, ic.case_ref(c, kind, s, F32), ic.F32_TOL, c.H, f'{ic.case_id(c)} {kind} s={s} fp32'))
    print(f'cross2 fp32 d{D}: worst per-slice error {worst:.2e} (bound {ic.F32_TOL})')


def test_cross2_many_query_tiles(dev):
    """Nq = 2100: the 512-query workgroups (four tiles per wave, the prefetched Q rows) with a ragged last workgroup and a ragged last tile."""
    c = ic.Case2(1, 2, 2100, 77, 4, 40, False)
    x = ic.case_inputs(c, 'image')
    e = ic.close_slices(run_cross2(x, 1.0, c.H, False, dev), ic.case_ref(c, 'image', 1.0), ic.FWD_TOL, c.H, ic.case_id(c))
    x32 = ic.case_inputs(c, 'image', F32)
    e32 = ic.close_slices(run_cross2(x32, 1.0, c.H, False, dev), ic.case_ref(c, 'image', 1.0, F32), ic.F32_TOL, c.H, ic.case_id(c) + ' fp32')
    print(f'cross2 q2100: bf16 {e:.5f}, fp32 {e32:.2e}')


def _raw(dtype, ps=False):
    from sid_lsg_amd._lib import lib
    name = 'sidlsg_attn_cross2_fwd' + ('_f32' if dtype == F32 else ('_ps' if ps else ''))
    return getattr(lib, name).raw


def _raw_call(fn, q, kv, view, o, s, H, Nq, Nk, Nk2, D, over=None):
    """The C entry point on the UNet's layout; `over` replaces single arguments (pointers as integers)."""
    C, es = H * D, q.element_size()
    a = dict(Q=q.data_ptr(), K=kv.data_ptr(), V=kv.data_ptr() + C * es, K2=view.data_ptr(), V2=view.data_ptr() + C * es, O=o.data_ptr(), s=s,
             B=q.shape[0], H=H, Nq=Nq, Nk=Nk, Nk2=Nk2, D=D, ldq=q.stride(1), ldk=kv.stride(1), ldv=kv.stride(1), ldk2=view.stride(1),
             ldv2=view.stride(1), ldo=o.stride(1), bsq=q.stride(0), bsk=kv.stride(0), bsv=kv.stride(0), bsk2=view.stride(0), bsv2=view.stride(0),
             bso=o.stride(0))
    a.update(over or {})
    rc = fn(*a.values(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'fp32'])
def test_cross2_layout_and_refusals(dev, dtype):
    from sid_lsg_amd import ops
    c = ic.Case2(2, 4, 130, 77, 4, 40, False)
    H, D, C = c.H, c.D, c.H * c.D
    tol = ic.FWD_TOL if dtype == BF16 else ic.F32_TOL
    x = ic.case_inputs(c, 'image', dtype)
    q, kv, view = device_operands(x, dev)
    fn = _raw(dtype)
    # O rows >= Nq are untouched: three sentinel rows behind every batch element's 130
    sentinel = 123.0
    o = torch.full((c.B, c.Nq + 3, C), sentinel, dtype=dtype, device=dev)
    assert _raw_call(fn, q, kv, view, o, 1.0, H, c.Nq, c.Nk, c.Nk2, D) == 0
    ic.close_slices(o[:, :c.Nq], ic.case_ref(c, 'image', 1.0, dtype), tol, H, 'padded O')
    assert bool((o[:, c.Nq:] == sentinel).all())
    # the wide buffer's NaN columns were never read; fewer queries than the buffer holds: rows >= Nq of Q are not needed either
    o2 = torch.full_like(o, sentinel)
    assert _raw_call(fn, q, kv, view, o2, 1.0, H, 17, c.Nk, c.Nk2, D) == 0
    assert torch.equal(o2[:, :17], o[:, :17]) and bool((o2[:, 17:] == sentinel).all())
    # s = 0: the one-set result of the same kernel, whatever K2 / V2 hold (they are not read), and the fp64 text attention
    with torch.no_grad():
        nan_view = torch.full_like(view, float('nan'))
        z1 = ops.cross_attention2(q, kv, view, H, 0.0)
        z2 = ops.cross_attention2(q, kv, nan_view, H, 0.0)
        plain = ops.cross_attention(q, kv, H)
    assert torch.equal(z1, z2) and torch.isfinite(z1).all()
    ic.close_slices(z1, ic.one_set_ref64(x, H), tol, H, 's = 0')
    ic.close_slices(z1, plain, 2 * tol, H, 's = 0 against sidlsg_attn_fwd')
    # every refused call returns SIDLSG_EINVAL and writes nothing
    o3 = torch.full_like(o, sentinel)
    es = q.element_size()
    refused = [dict(Nk=0), dict(Nk=129), dict(Nk2=0), dict(Nk2=33), dict(Nq=0), dict(D=0), dict(D=168), dict(D=D + 2), dict(H=0), dict(B=0),
               dict(Q=0), dict(K2=0), dict(V2=0), dict(O=0), dict(K2=view.data_ptr() + es), dict(Q=q.data_ptr() + 2 * es), dict(ldk2=view.stride(1) + 1),
               dict(ldv2=C - 8), dict(ldo=C + 2), dict(bsk2=view.stride(0) + 1), dict(bso=-o.stride(0)), dict(s=float('nan')), dict(s=float('inf'))]
    refused += [dict(D=4)] if dtype == BF16 else [dict(Nk=128, Nk2=32, D=160, H=1)]
    for over in refused:
        assert _raw_call(fn, q, kv, view, o3, 1.0, H, c.Nq, c.Nk, c.Nk2, D, over) == EINVAL, over
    if dtype == BF16:
        for over in refused[:6]:
            assert _raw_call(_raw(dtype, ps=True), q, kv, view, o3, 1.0, H, c.Nq, c.Nk, c.Nk2, D, over) == EINVAL, over
    assert bool((o3 == sentinel).all())
    # the Python side says why
    with torch.no_grad():
        for bad, match in ((view[:, :, :2 * C - 8], 'expected'), (torch.cat([view] * 9, 1), 'image keys'), (view.float() if dtype == BF16 else view.to(BF16), 'must be')):
            with pytest.raises(RuntimeError, match=match):
                ops.cross_attention2(q, kv, bad, H, 1.0)
        with pytest.raises(RuntimeError, match='text keys'):
            ops.cross_attention2(q, torch.cat([kv, kv], 1), view, H, 1.0)
        with pytest.raises(RuntimeError, match='head width'):
            ops.cross_attention2(q, kv, view, 16, 1.0)
        with pytest.raises(RuntimeError, match='not finite'):
            ops.cross_attention2(q, kv, view, H, float('nan'))
    with pytest.raises(RuntimeError, match='forward only'):
        ops.cross_attention2(q.clone().requires_grad_(True), kv, view, H, 1.0)


# ---- 4 - 9. adapter, UNet, samplers ---------------------------------------------------------------------------------------------------
_refs, _nets = {}, {}


def ref_set(name):
    """(ControlledUNetRef with IP attn2, IPAdapterRef, unet state dict, adapter state dict) in fp64, built once per configuration."""
    if name not in _refs:
        _refs[name] = ir.make_ref(name)
    return _refs[name]


def hip_set(name, cd, dev):
    """(HipUNet2DCondition, HipIPAdapter) of compute dtype `cd` holding the reference's weights, built once."""
    from sid_lsg_amd.ip_adapter import HipIPAdapter
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    if (name, cd) not in _nets:
        _, _, usd, isd = ref_set(name)
        unet = HipUNet2DCondition(CONFIGS[name], compute_dtype=cd).materialize(dev, with_grad_buffers=False, source=usd).requires_grad_(False)
        _nets[(name, cd)] = (unet, HipIPAdapter(CONFIGS[name], isd, dev, cd, ir.EMBED_DIM))
    return _nets[(name, cd)]


def nhwc8(x, cd, dev):
    B, C, h, w = x.shape
    out = torch.zeros(B, h, w, 8)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out.to(cd).to(dev)


def nchw(eps, h, w):
    return eps.view(eps.shape[0], h, w, 8)[..., :4].permute(0, 3, 1, 2).cpu()


def run_unet(unet, x, t, ctx, dev, **kw):
    """One pass on CPU inputs -> [B, 4, h, w] on the CPU; without a state the call has no `ip` / `control` argument at all."""
    h, w = x.shape[2:]
    with torch.no_grad():
        eps = unet.forward_nhwc(nhwc8(x, unet.compute_dtype, dev), t.to(dev), ctx.to(unet.compute_dtype).to(dev).contiguous(), **kw)
    return nchw(eps, h, w)


@pytest.mark.parametrize('name', ['tiny40', 'tiny21'])
def test_prepare_matches_the_reference_f32(dev, name):
    """Tokens and every layer's K2 / V2, fp32 mode, 1e-4 of max |ref|; the dup = 2 uncond half is the projection of zero embeddings."""
    _, ad, _, _ = ref_set(name)
    _, hip = hip_set(name, F32, dev)
    _, _, _, emb = ir.make_inputs(name)
    with torch.no_grad():
        want_tok = ad.image_proj(emb.double())
        want_kv = ad.layer_kv(want_tok)
        want_zero = ad.image_proj(torch.zeros_like(emb).double())
    state = hip.prepare(emb.to(dev), 1.0)
    assert state.tokens.shape == (3, ir.TOKENS, want_tok.shape[-1]) and state.tokens.dtype == F32 and state.kv.shape == (3, ir.TOKENS, hip.width)
    worst = close(state.tokens, want_tok, FP32_TOL, 'tokens')
    assert len(want_kv) == len(hip.channels) == 16
    for i, (k, v) in enumerate(want_kv):
        view = state.layer_kv(i)
        assert view.shape == (3, ir.TOKENS, 2 * hip.channels[i]) and view.stride(1) == hip.width and view.data_ptr() % 16 == 0
        worst = max(worst, close(view[..., :hip.channels[i]], k, FP32_TOL, f'K2 of layer {i}'), close(view[..., hip.channels[i]:], v, FP32_TOL, f'V2 of layer {i}'))
    two = hip.prepare(emb.to(dev), 0.5, dup=2)
    zero = hip.prepare(torch.zeros_like(emb).to(dev), 0.5)
    assert two.kv.shape[0] == 6 and two.scale == 0.5
    assert torch.equal(two.tokens[:3], zero.tokens) and torch.equal(two.kv[:3], zero.kv)
    assert torch.equal(two.tokens[3:], state.tokens) and torch.equal(two.kv[3:], state.kv)
    close(two.tokens[:3], want_zero, FP32_TOL, 'uncond tokens')
    assert float(zero.tokens.abs().max()) > 0.1                       # bias and LayerNorm still act
    print(f'{name}: tokens and 16 x (K2, V2), fp32 mode: worst max-norm error {worst:.2e}')
    for bad, match in ((emb[:, :16].to(dev), 'expected'), (emb, 'GPU only')):
        with pytest.raises((ValueError, RuntimeError), match=match):
            hip.prepare(bad, 1.0)
    for kw in (dict(scale=-1.0), dict(scale=float('nan')), dict(dup=3)):
        with pytest.raises(ValueError):
            hip.prepare(emb.to(dev), **kw)


@pytest.mark.parametrize('scale', [1.0, 0.5])
@pytest.mark.parametrize('name', ['tiny40', 'tiny21'])
def test_unet_with_image_prompt_matches_the_reference_f32(dev, name, scale):
    uref, ad, _, _ = ref_set(name)
    unet, hip = hip_set(name, F32, dev)
    x, t, ctx, emb = ir.make_inputs(name)
    plain, want = ir.ref_outputs(uref, ad, x, t, ctx, emb, scale)
    got = run_unet(unet, x, t, ctx, dev, ip=hip.prepare(emb.to(dev), scale))
    e = close(got, want, FP32_TOL, 'image-prompted UNet')
    print(f'{name} scale {scale}: image-prompted UNet, fp32 mode: max-norm error {e:.2e}; image-prompt effect {rel_l2(want, plain):.3f}')
    assert rel_l2(got, plain) > 0.05


@pytest.mark.parametrize('name', ['tiny40', 'tiny21'])
def test_unet_with_image_prompt_bf16_error_is_at_most_twice_the_plain_error(dev, name):
    """Relative l2 error against fp64 of the image-prompted bf16 output <= 2 x that of the UNCHANGED plain bf16 UNet on the same inputs
    (the rule of the ControlNet test).  Both figures are printed (-s).  Measured on an MI355X (profiles/ip_adapter.txt): tiny40 plain
    9.567e-3, image-prompted 9.093e-3 (0.95 x); tiny21 plain 1.112e-2, image-prompted 9.964e-3 (0.90 x)."""
    uref, ad, _, _ = ref_set(name)
    unet, hip = hip_set(name, BF16, dev)
    x, t, ctx, emb = ir.make_inputs(name)
    plain, want = ir.ref_outputs(uref, ad, x, t, ctx, emb, 1.0)
    e_plain = rel_l2(run_unet(unet, x, t, ctx, dev), plain)
    got = run_unet(unet, x, t, ctx, dev, ip=hip.prepare(emb.to(dev), 1.0))
    e_ip = rel_l2(got, want)
    print(f'{name} bf16: plain UNet rel l2 {e_plain:.3e}, image-prompted {e_ip:.3e}, ratio {e_ip / e_plain:.2f}')
    assert torch.isfinite(got).all() and e_plain > 0
    assert e_ip <= 2 * e_plain


class _CallCounter:
    """Counts the calls of every C entry point by wrapping the binding's cached callables (restored on exit)."""

    def __enter__(self):
        from sid_lsg_amd._lib import lib
        self.lib, self.counts, self.saved = lib, collections.Counter(), {}
        for name in lib.protos:
            fn = getattr(lib, name)
            self.saved[name] = fn

            def counted(*a, _fn=fn, _name=name):
                self.counts[_name] += 1
                return _fn(*a)
            counted.raw = fn.raw
            lib.__dict__[name] = counted
        return self.counts

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            self.lib.__dict__[name] = fn


@pytest.mark.parametrize('cd', [BF16, F32], ids=['bf16', 'fp32'])
def test_exactness_and_launch_count(dev, cd):
    name = 'tiny40'
    unet, hip = hip_set(name, cd, dev)
    x, t, ctx, emb = ir.make_inputs(name)
    xin, tt, cc = nhwc8(x, cd, dev), t.to(dev), ctx.to(cd).to(dev).contiguous()
    state, state0 = hip.prepare(emb.to(dev), 1.0), hip.prepare(emb.to(dev), 0.0)
    with torch.no_grad():
        unet.forward_nhwc(xin, tt, cc)                    # one-off calls (workspace, compute copies) happen outside the counts
        unet.forward_nhwc(xin, tt, cc, ip=state)
        with _CallCounter() as n_plain:
            plain = unet.forward_nhwc(xin, tt, cc)
        with _CallCounter() as n_ip:
            full = unet.forward_nhwc(xin, tt, cc, ip=state)
        with _CallCounter() as n_zero:
            zero = unet.forward_nhwc(xin, tt, cc, ip=state0)
        assert torch.equal(unet.forward_nhwc(xin, tt, cc, ip=None), plain) and torch.equal(unet.forward_nhwc(xin, tt, cc, None, None), plain)
    assert torch.equal(zero, plain) and not torch.equal(full, plain) and torch.isfinite(full).all()
    one = 'sidlsg_attn_fwd' + ('_f32' if cd == F32 else '_ps' if unet.mid_block.attentions[0].transformer_blocks[0].attn2.prescaled else '')
    two = one.replace('attn_fwd', 'attn_cross2_fwd')
    fwd = lambda n: sum(v for k, v in n.items() if k.startswith('sidlsg_attn_fwd'))      # noqa: E731
    assert n_ip[two] == 16 and n_plain[two] == 0 and fwd(n_plain) == 32 and fwd(n_ip) == 16 and n_plain[one] - n_ip[one] == 16      # 16 attn1 + 16 attn2
    moved = collections.Counter(n_ip)
    moved[one] += moved.pop(two)
    assert moved == n_plain, f'the image-prompt pass issues other library calls than the plain pass: {moved - n_plain} / {n_plain - moved}'
    assert sum(n_ip.values()) == sum(n_plain.values())
    assert n_zero == n_plain
    assert all(m.ip is None for m in unet.cross_attention_layers())          # nothing stays bound after a pass
    # dup = 2: the uncond rows do not depend on the image
    g = torch.Generator().manual_seed(3)
    emb2 = torch.randn(emb.shape, generator=g)
    x2, t2, c2 = torch.cat([xin, xin]), torch.cat([tt, tt]), torch.cat([cc, cc])
    with torch.no_grad():
        a = unet.forward_nhwc(x2, t2, c2, ip=hip.prepare(emb.to(dev), 1.0, dup=2))
        b = unet.forward_nhwc(x2, t2, c2, ip=hip.prepare(emb2.to(dev), 1.0, dup=2))
    assert torch.equal(a[:3], b[:3]) and not torch.equal(a[3:], b[3:]) and torch.isfinite(a).all()


@pytest.mark.parametrize('name', ['tiny40'])
def test_image_prompt_composes_with_a_controlnet_f32(dev, name):
    """ip + control against the reference with both applied; the ControlNet sees the text only."""
    from sid_lsg_amd.controlnet import HipControlNet
    from sid_lsg_amd.unet import CONFIGS
    uref, ad, _, _ = ref_set(name)
    unet, hip = hip_set(name, F32, dev)
    _, cnet, _, csd = cr.make_pair(name)
    net = HipControlNet(CONFIGS[name], compute_dtype=F32).materialize(dev, source=csd)
    x, t, ctx, emb = ir.make_inputs(name)
    img = torch.randint(0, 256, (3, 64, 128, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    with torch.no_grad():
        ad.set(None)
        res = cnet(x.double(), t, ctx.double(), (img.double() / 255).permute(0, 3, 1, 2), 0.8)
    plain_c, want = ir.ref_outputs(uref, ad, x, t, ctx, emb, 0.6, residuals=res)
    plain, only_ip = ir.ref_outputs(uref, ad, x, t, ctx, emb, 0.6)
    got = run_unet(unet, x, t, ctx, dev, control=net.prepare(img.to(dev), 0.8), ip=hip.prepare(emb.to(dev), 0.6))
    e = close(got, want, FP32_TOL, 'ip + control')
    print(f'{name}: ip + control, fp32 mode: max-norm error {e:.2e}; against control only {rel_l2(want, plain_c):.3f}, against ip only {rel_l2(want, only_ip):.3f}')
    assert rel_l2(got, plain_c) > 0.05 and rel_l2(got, only_ip) > 0.05


PROMPTS = ['a red cube on a table', 'two blue spheres']
_model = {}


def model(dev, cd):
    """random:tiny with its text encoder, tokenizer and scheduler, a seeded adapter for it and two image embeddings."""
    if cd not in _model:
        from sid_lsg_amd.sd_util import load_ip_adapter, load_sd15
        unet, vae, sched, te, tok = load_sd15('random:tiny', None, dev, F32, compute_dtype=cd)
        unet.eval().requires_grad_(False)
        hip = load_ip_adapter('random:ip-adapter:3', unet, dev, ir.EMBED_DIM)
        emb = torch.randn(2, ir.EMBED_DIM, generator=torch.Generator().manual_seed(4)).to(dev)
        _model[cd] = (unet, sched, te, tok, hip, emb)
    return _model[cd]


def _z(dev, seed=11):
    return torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(seed)).to(dev)


@pytest.mark.parametrize('solver', ['ddim', 'dpmpp2m'])
def test_one_guided_teacher_step_matches_the_loop_on_the_reference(dev, solver):
    """One guided step (N = 1) of teacher_sample_i2i / teacher_sample_solver_i2i in the fp32 mode against the same step written out on the
    fp64 reference: e = u + kappa (c - u) with the [uncond ; cond] text states and the [proj(0) ; proj(e)] image tokens, x0 = (x - s1 e) /
    s0, x' = a x + b e.  Bound: the UNet's fp32-mode bound FP32_TOL on each of u and c, i.e. (1 + 2 kappa) FP32_TOL max|eps_ref| |b| on x'
    (computed from reference values), plus 1e-5 max|x'| for the fp32 step arithmetic."""
    from sid_lsg_amd.scheduler import ddim_schedule, solver_schedule
    from sid_lsg_amd.sd_util import encode_contexts, sampling_config_of, teacher_sample_i2i, teacher_sample_solver_i2i
    unet, sched, te, tok, hip, emb = model(dev, F32)
    z, kappa, b = _z(dev), 2.5, 2
    state = hip.prepare(emb, 0.7, dup=2)
    if solver == 'ddim':
        got = teacher_sample_i2i(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=kappa, num_inference_steps=1, ip=state)
        plain = teacher_sample_i2i(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=kappa, num_inference_steps=1)
        ts, s0, s1, s0p, s1p = (v.double().cpu() for v in ddim_schedule(sched, sampling_config_of(sched), 1))
        ca, cb = float(s0p[0] / s0[0]), float(s1p[0] - s0p[0] * s1[0] / s0[0])
    else:
        kw = dict(guidance_scale=kappa, num_inference_steps=1, solver='dpmpp2m')
        got = teacher_sample_solver_i2i(unet, z, PROMPTS, sched, te, tok, 64, ip=state, **kw)
        plain = teacher_sample_solver_i2i(unet, z, PROMPTS, sched, te, tok, 64, **kw)
        ts, s0, s1, coef = (v.double().cpu() for v in solver_schedule(sched, sampling_config_of(sched), 1, solver='dpmpp2m', spacing=None, eta=0.0, start=0))
        assert float(coef[0, 2]) == 0 and float(coef[0, 3]) == 0
        ca, cb = float(coef[0, 0] + coef[0, 1] / s0[0]), float(-coef[0, 1] * s1[0] / s0[0])
    key = ('teacher-ref',)
    if key not in _refs:
        _refs[key] = ir.make_ref('tiny', adapter_seed=3, usd=unet.state_dict())
    uref, ad, _, isd = _refs[key]
    assert all(torch.equal(v, hip.state_dict()[k]) for k, v in isd.items())
    with torch.no_grad():
        ctx = torch.cat([encode_contexts([''] * b, te, tok, dev), encode_contexts(PROMPTS, te, tok, dev)]).double().cpu()
        ad.set(ad.image_proj(torch.cat([torch.zeros_like(emb), emb]).double().cpu()), 0.7)
        x = z.double().cpu()
        eps = uref(torch.cat([x, x]), ts[0].long().expand(2 * b), encoder_hidden_states=ctx).sample
        ad.set(None)
    e = eps[:b] + kappa * (eps[b:] - eps[:b])
    want = ca * x + cb * e
    bound = (1 + 2 * kappa) * FP32_TOL * float(eps.abs().max()) * abs(cb) + 1e-5 * float(want.abs().max())
    err = float((got.double().cpu() - want).abs().max())
    print(f'{solver}: one guided step with an image prompt, fp32 mode: max err {err:.3e}, bound {bound:.3e}; effect of the prompt {rel_l2(got, plain.cpu()):.3f}')
    assert torch.isfinite(got).all() and err <= bound
    assert rel_l2(got, plain.cpu()) > 10 * bound / float(want.abs().max())


def test_teacher_samplers_with_ip_are_the_hand_written_loops(dev):
    """Three guided steps, bf16: the samplers pass the state to every UNet call and change nothing else; scale 0 is the plain sampler."""
    from sid_lsg_amd import ops
    from sid_lsg_amd.scheduler import ddim_schedule
    from sid_lsg_amd.sd_util import encode_contexts, sampling_config_of, teacher_sample, teacher_sample_i2i, teacher_sample_solver, teacher_sample_solver_i2i
    unet, sched, te, tok, hip, emb = model(dev, BF16)
    z, N, kappa, b = _z(dev), 3, 2.5, 2
    state = hip.prepare(emb, 1.0, dup=2)
    got = teacher_sample_i2i(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=kappa, num_inference_steps=N, ip=state)
    plain = teacher_sample(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=kappa, num_inference_steps=N)
    with torch.no_grad():
        ts, s0, s1, s0p, s1p = (v.to(dev) for v in ddim_schedule(sched, sampling_config_of(sched), N))
        row = lambda v, i: v.to(F32)[i].expand(b).contiguous()      # noqa: E731
        ctx = torch.cat([encode_contexts([''] * 2, te, tok, dev), encode_contexts(PROMPTS, te, tok, dev)]).to(BF16).contiguous()
        ones = torch.ones(b, device=dev)
        xin, xt = ops.noisy_input(None, z, ones, ones, 2, BF16)
        for i in range(N):
            eps = unet.forward_nhwc(xin, ts[i].expand(2 * b).contiguous(), ctx, ip=state)
            xin, xt, _ = ops.ddim_step(eps, xt, row(s0, i), row(s1, i), row(s0p, i), row(s1p, i), kappa, BF16, prediction_type='epsilon', last=i == N - 1)
    torch.cuda.synchronize()
    assert torch.equal(got, xt) and torch.isfinite(got).all() and not torch.equal(got, plain)
    assert torch.equal(teacher_sample_i2i(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=kappa, num_inference_steps=N,
                                          ip=hip.prepare(emb, 0.0, dup=2)), plain)
    kw = dict(guidance_scale=kappa, num_inference_steps=N, solver='dpmpp2m')
    sol = teacher_sample_solver_i2i(unet, z, PROMPTS, sched, te, tok, 64, ip=state, **kw)
    sol_plain = teacher_sample_solver(unet, z, PROMPTS, sched, te, tok, 64, **kw)
    assert torch.isfinite(sol).all() and not torch.equal(sol, sol_plain)
    assert torch.equal(teacher_sample_solver_i2i(unet, z, PROMPTS, sched, te, tok, 64, ip=hip.prepare(emb, 0.0, dup=2), **kw), sol_plain)


@pytest.mark.parametrize('steps', [1, 2])
def test_sid_sd_sampler_with_ip(dev, steps):
    from sid_lsg_amd import ops
    from sid_lsg_amd.sd_util import encode_contexts, sid_sd_sampler
    unet, sched, te, tok, hip, emb = model(dev, BF16)
    z = _z(dev)
    init_t = torch.full((2,), 625, dtype=torch.long, device=dev)
    state = hip.prepare(emb, 1.0, dup=1)
    kw = dict(unet=unet, latents=z, contexts=PROMPTS, init_timesteps=init_t, noise_scheduler=sched, text_encoder=te, tokenizer=tok, resolution=64,
              train_sampler=False, num_steps_eval=steps)
    torch.manual_seed(5)
    got = sid_sd_sampler(ip=state, **kw)
    torch.manual_seed(5)
    plain = sid_sd_sampler(**kw)
    torch.manual_seed(5)
    with torch.no_grad():
        emb_t = encode_contexts(PROMPTS, te, tok, dev).to(BF16).contiguous()
        D = None
        for i in range(steps):
            noise = z if i == 0 else torch.randn_like(z)
            t_i = (init_t * (1 - i / steps)).to(torch.long).contiguous()
            s0, s1 = sched.coefficients(t_i)
            xin, xt = ops.noisy_input(D, noise.to(F32).contiguous(), s0, s1, 1, BF16)
            eps = unet.forward_nhwc(xin, t_i, emb_t, ip=state)
            D = ops.cfg_x0(eps, xt, s0, s1, 1.0, True, BF16, prediction_type='epsilon')
    torch.cuda.synchronize()
    assert torch.equal(got, D.to(F32))
    assert torch.isfinite(got).all() and not torch.equal(got, plain)
    torch.manual_seed(5)
    assert torch.equal(sid_sd_sampler(ip=hip.prepare(emb, 0.0), **kw), plain)
    with pytest.raises(ValueError, match='train_sampler=False'):
        sid_sd_sampler(**dict(kw, train_sampler=True, ip=state))


def test_refusals_on_the_gpu(dev):
    from sid_lsg_amd import ip_adapter as ipa
    from sid_lsg_amd import ops
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    name = 'tiny'
    cfg = CONFIGS[name]
    unet = HipUNet2DCondition(cfg, compute_dtype=BF16).materialize(dev, with_grad_buffers=False, seed=1).requires_grad_(False)
    hip = ipa.load_ip_adapter('random:ip-adapter', unet, dev, ir.EMBED_DIM)
    x, t, ctx, _ = cr.make_inputs(name, w=16)
    emb = torch.randn(3, ir.EMBED_DIM, generator=torch.Generator().manual_seed(1)).to(dev)
    state = hip.prepare(emb, 1.0)
    xin, tt, cc = nhwc8(x, BF16, dev), t.to(dev), ctx.to(BF16).to(dev)
    with pytest.raises(RuntimeError, match='autograd'):
        unet.forward_nhwc(xin, tt, cc, ip=state)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='grouped pass'):
            with ops.dual_networks({}):
                unet.forward_nhwc(xin, tt, cc, ip=state)
        with pytest.raises(ValueError, match='dup'):                           # a guided batch with a dup = 1 state
            unet.forward_nhwc(torch.cat([xin, xin]), torch.cat([tt, tt]), torch.cat([cc, cc]), ip=state)
        with pytest.raises(ValueError, match='rows'):
            unet.forward_nhwc(xin[:2].contiguous(), tt[:2], cc[:2].contiguous(), ip=state)
        f32 = ipa.HipIPAdapter(cfg, hip.state_dict(), dev, F32, ir.EMBED_DIM)
        with pytest.raises(RuntimeError, match='computes in'):
            unet.forward_nhwc(xin, tt, cc, ip=f32.prepare(emb, 1.0))

        def other(**change):
            c = dataclasses.replace(cfg, **change)
            net = HipUNet2DCondition(c, compute_dtype=BF16).materialize(dev, with_grad_buffers=False, seed=2).requires_grad_(False)
            return net, torch.zeros(3, c.text_len, c.cross_attention_dim, dtype=BF16, device=dev)
        net, c2 = other(cross_attention_dim=128)
        with pytest.raises(ValueError, match='cross_attention_dim'):
            net.forward_nhwc(xin, tt, c2, ip=state)
        net, c2 = other(down_has_attn=(True, True, False, False))
        with pytest.raises(ValueError, match='16 layers, the UNet 11 cross-attention layers'):
            net.forward_nhwc(xin, tt, c2, ip=state)
        net, c2 = other(block_out_channels=(32, 64, 64, 128))
        with pytest.raises(ValueError, match='channels'):
            net.forward_nhwc(xin, tt, c2, ip=state)
        assert all(m.ip is None for m in unet.cross_attention_layers())
        fp8 = HipUNet2DCondition(cfg, compute_dtype=BF16).materialize(dev, with_grad_buffers=False, seed=1).requires_grad_(False)
        fp8.enable_fp8_weights()
        with pytest.raises(RuntimeError, match='e4m3'):
            fp8.forward_nhwc(xin, tt, cc, ip=state)
    with pytest.raises(ValueError, match='projection_dim 64'):
        ipa.load_ip_adapter('random:ip-adapter', unet, dev, 32).prepare_images(
            torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device=dev),
            type('T', (), dict(preprocess='pil', cfg=type('C', (), dict(projection_dim=64))))())
    with pytest.raises(ValueError, match="preprocess='pil'"):
        hip.prepare_images(torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device=dev), type('T', (), dict(preprocess='interpolate'))())


def test_prepare_images_runs_the_pil_tower(dev):
    from sid_lsg_amd.clip import load_clip_vision
    unet, _, _, _, hip, _ = model(dev, BF16)
    tower = load_clip_vision('random:clip-tiny', dev, BF16)
    assert tower.preprocess == 'pil' and tower.cfg.projection_dim == ir.EMBED_DIM
    img = torch.randint(0, 256, (2, 3, 40, 56), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).to(dev)
    with torch.no_grad():
        e = tower(img).float()
    a, b = hip.prepare_images(img, tower, 0.5, dup=2), hip.prepare(e, 0.5, dup=2)
    assert torch.equal(a.kv, b.kv) and a.kv.shape[0] == 4 and torch.isfinite(a.kv).all() and not torch.equal(a.kv[2], a.kv[3])


# ---- 10. command line ----------------------------------------------------------------------------------------------------------------------
def _png_pixels(path):
    import PIL.Image
    return np.asarray(PIL.Image.open(path).convert('RGB'))


def test_generate_onestep_with_an_ip_adapter(dev, tmp_path):
    """`generate_onestep.py --network teacher --ip_adapter random:ip-adapter --ip_image_encoder random:clip-tiny --ip_images DIR`, 3 steps, in a
    child process; then, in this process, the run without the options and the run at --ip_scale 0: the PNGs exist, differ from the plain
    run's, and are identical to it at scale 0."""
    import PIL.Image
    from click.testing import CliRunner
    import generate_onestep
    prompts = tmp_path / 'prompts.txt'
    prompts.write_text('a red cube\na blue sphere\n')
    pics = tmp_path / 'pics'
    pics.mkdir()
    g = torch.Generator().manual_seed(2)
    for i, (h, w) in enumerate(((48, 72), (90, 60))):                        # any size: the 'pil' transform resizes
        PIL.Image.fromarray(torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy()).save(str(pics / f'ref{i}.png'))
    common = ['--network', 'teacher', '--repo_id', 'random:tiny', '--teacher_steps', '3', '--seeds', '0-1', '--resolution', '64',
              '--text_prompts', str(prompts)]
    ip = ['--ip_adapter', 'random:ip-adapter', '--ip_image_encoder', 'random:clip-tiny', '--ip_images', str(pics)]
    with socket.socket() as sock:           # a rendezvous port of the child's own: this process may hold the default one
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    out_a, out_z, out_p = tmp_path / 'a', tmp_path / 'z', tmp_path / 'plain'
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'generate_onestep.py'), '--outdir', str(out_a)] + common + ip,
                         cwd=ROOT, capture_output=True, text=True, timeout=240, env=dict(os.environ, MASTER_PORT=str(port)))
    assert res.returncode == 0, res.stdout + res.stderr
    assert 'IP-Adapter "random:ip-adapter": 4 image tokens, scale 1' in res.stdout
    r2 = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out_z)] + common + ip + ['--ip_scale', '0'], catch_exceptions=False)
    assert r2.exit_code == 0 and 'scale 0,' in r2.output, r2.output
    r3 = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out_p)] + common, catch_exceptions=False)
    assert r3.exit_code == 0 and 'IP-Adapter' not in r3.output, r3.output
    r4 = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out_p)] + common + ip[:2])
    assert r4.exit_code == 2 and '--ip_image_encoder' in r4.output
    names = ['000000.png', '000001.png']
    pix = {}
    for d in (out_a, out_z, out_p):
        assert [os.path.basename(f) for f in sorted(glob.glob(str(d / '*.png')))] == names
        pix[d] = [_png_pixels(str(d / n)) for n in names]
    for a, z, p in zip(pix[out_a], pix[out_z], pix[out_p]):
        assert a.shape == (64, 64, 3) and a.min() != a.max()
        assert np.array_equal(z, p) and not np.array_equal(a, p)
