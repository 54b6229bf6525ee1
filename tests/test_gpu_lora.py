"""LoRA on the GPU: the merge kernel (csrc/lora.hip) on exact integer cases, on float cases against fp64 under the derived fma-chain
bound and on everything it must refuse; the bookkeeping of lora.LoraSet / lora.fuse on random:tiny against the independent fp64
restatement of tests/lora_ref.py; the adapted UNet and text encoder; the launch count of a pass; the command lines.

The float bound, per element:  |got - ref| <= (R + 3) 2^-24 (|base| + sum_r |coef up down|)  -- the standard bound of an fp32 fma
chain of length R (gamma_R), one more rounding for the product coef * up and one for the final add of base.  It is derived, not
measured; the worst observed ratio to it is printed (-s; profiles/lora.txt keeps a run)."""
import collections
import glob
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import lora_ref

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
FP32_TOL = 1e-4      # max |err| / max |ref| of the fp32-mode UNet: FP32_TOL of tests/test_gpu_controlnet.py and tests/test_gpu_ip_adapter.py
U = 2.0 ** -24


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
INT_SHAPES = [(4, 2880, 4), (320, 36, 8), (24, 72, 4), (130, 260, 12), (64, 64, 64)]


def int_case(N, KK, R, salt=0, needle=None):
    """Small integers (|v| <= 8) that depend on BOTH indices, coefficients 1, 2, 4 by column; `needle`: that column's coefficient times 2^10."""
    n, k, r = torch.arange(N)[:, None], torch.arange(KK)[None, :], torch.arange(R)
    base = ((n * 7 + k * 3 + salt) % 17 - 8).float()
    up = ((n * 5 + r[None, :] * 11 + salt) % 13 - 6).float()
    down = ((r[:, None] * 3 + k * 7 + 2 * salt) % 15 - 7).float()
    coef = (2.0 ** (r % 3)).float()
    if needle is not None:
        coef[needle] *= 1024.0
    ref = base.long() + (up.long() * coef.long()) @ down.long()
    assert int(ref.abs().max()) < 1 << 24 and float(up.abs().max()) <= 8 and float(down.abs().max()) <= 8 and float(base.abs().max()) <= 8
    return base, up, down, coef, ref


def launch(dev, cases, in_place=False, dst_fill=float('nan')):
    """cases: [(base, up, down, coef)] CPU fp32 -> one launch over all of them -> [dst] on the device (dst is base's buffer when in_place)."""
    from sid_lsg_amd import ops
    keep, recs, dsts = [], [], []
    for base, up, down, coef in cases:
        b, u, d, c = (t.to(dev).contiguous() for t in (base, up, down, coef))
        dst = b if in_place else torch.full_like(b, dst_fill)
        keep += [b, u, d, c]
        dsts.append(dst)
        recs.append((b.data_ptr(), dst.data_ptr(), u.data_ptr(), d.data_ptr(), c.data_ptr(), base.shape[0], base.shape[1], up.shape[1]))
    table = ops.LoraJobTable(recs, dev)
    ops.lora_merge(table)
    torch.cuda.synchronize()
    return dsts


def test_integer_cases_all_in_one_launch_and_alone(dev):
    cases = [int_case(*s, salt=i) for i, s in enumerate(INT_SHAPES)]
    together = launch(dev, [c[:4] for c in cases])
    for s, c, got in zip(INT_SHAPES, cases, together):
        assert torch.equal(got.cpu().long(), c[4]) and torch.isfinite(got).all(), f'{s} in the joint launch'
        alone = launch(dev, [c[:4]])[0]
        assert torch.equal(alone.cpu().long(), c[4]), f'{s} alone'
        assert torch.equal(alone, got)
    # the jobs in another order (other blk0 of every job): the same results
    back = launch(dev, [c[:4] for c in reversed(cases)])
    for c, got in zip(reversed(cases), back):
        assert torch.equal(got.cpu().long(), c[4])


@pytest.mark.parametrize('shape, col', [((130, 260, 12), 7), ((64, 64, 64), 33), ((4, 2880, 4), 0)])
def test_needle_column(dev, shape, col):
    """One rank column weighs 2^10 times the others: a dropped or doubled rank step is an O(1) error, and the exact result must hold."""
    base, up, down, coef, ref = int_case(*shape, salt=3, needle=col)
    got = launch(dev, [(base, up, down, coef)])[0]
    assert torch.equal(got.cpu().long(), ref)
    plain = int_case(*shape, salt=3)[4]
    assert int((ref - plain).abs().max()) >= 1024


def test_in_place_and_twice_bit_for_bit(dev):
    base, up, down, coef, ref = int_case(130, 260, 12, salt=5)
    got = launch(dev, [(base, up, down, coef)], in_place=True)[0]
    assert torch.equal(got.cpu().long(), ref)
    g = torch.Generator().manual_seed(0)
    fb, fu, fd, fc = torch.randn(130, 260, generator=g), torch.randn(130, 12, generator=g), torch.randn(12, 260, generator=g), torch.randn(12, generator=g)
    a = launch(dev, [(fb, fu, fd, fc)])[0]
    b = launch(dev, [(fb, fu, fd, fc)])[0]
    c = launch(dev, [(fb, fu, fd, fc)], in_place=True)[0]
    assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize('N, KK, R', [(320, 2880, 128), (77, 768, 260)])
def test_float_cases_within_the_fma_chain_bound(dev, N, KK, R):
    g = torch.Generator().manual_seed(N + R)
    base, up, down, coef = torch.randn(N, KK, generator=g), torch.randn(N, R, generator=g), torch.randn(R, KK, generator=g), torch.randn(R, generator=g)
    got = launch(dev, [(base, up, down, coef)])[0].cpu().double()
    cu = up.double() * coef.double()
    ref = base.double() + cu @ down.double()
    mag = base.double().abs() + cu.abs() @ down.double().abs()
    ratio = float(((got - ref).abs() / ((R + 3) * U * mag)).max())
    print(f'lora merge ({N}, {KK}, {R}): worst |got - ref| / bound = {ratio:.4f} (bound (R + 3) 2^-24 (|base| + sum |coef up down|))')
    assert torch.isfinite(got).all() and ratio <= 1.0


def _raw(dev, rec_edit=None, nblocks=None, njobs=None, shape=(24, 72, 4)):
    """The raw entry point on one valid job, with one field of the record (or a launch argument) replaced -> (code, dst unchanged?)."""
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    base, up, down, coef, _ = int_case(*shape)
    b, u, d, c = (t.to(dev).contiguous() for t in (base, up, down, coef))
    dst = torch.full((shape[0] * shape[1] + 64,), -3.0, device=dev)
    table = ops.LoraJobTable([(b.data_ptr(), dst.data_ptr(), u.data_ptr(), d.data_ptr(), c.data_ptr(), shape[0], shape[1], shape[2])], dev)
    rec = table.host.copy()
    if rec_edit:
        for k, v in rec_edit.items():
            rec[k][0] = v if not callable(v) else v(int(rec[k][0]))
    devrec = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    code = lib.sidlsg_lora_merge_f32.raw(rec.ctypes.data, devrec.data_ptr(), table.njobs if njobs is None else njobs,
                                         table.nblocks if nblocks is None else nblocks, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, bool((dst == -3.0).all())


@pytest.mark.parametrize('edit', [
    dict(base=lambda p: p + 4), dict(dst=lambda p: p + 8), dict(up=lambda p: p + 4), dict(down=lambda p: p + 12), dict(coef=lambda p: p + 4),
    dict(base=0), dict(KK=70), dict(KK=0), dict(R=6), dict(R=0), dict(R=4100), dict(N=0), dict(N=1 << 15, KK=1 << 14), dict(blk0=1),
], ids=lambda e: ','.join(e))
def test_einval_before_any_launch(dev, edit):
    code, untouched = _raw(dev, edit)
    assert code == EINVAL and untouched


def test_einval_table_level(dev):
    assert _raw(dev)[0] == 0                                  # the unedited call is accepted
    for kw in (dict(nblocks=1), dict(nblocks=3), dict(njobs=0), dict(nblocks=0)):
        code, untouched = _raw(dev, None, **kw)
        assert code == EINVAL and untouched, kw
    # two jobs out of order
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    cases = [int_case(24, 72, 4), int_case(64, 64, 64)]
    keep, recs = [], []
    for base, up, down, coef, _ in cases:
        t = [x.to(dev).contiguous() for x in (base, torch.full_like(base, -3.0), up, down, coef)]
        keep.append(t)
        recs.append((t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), base.shape[0], base.shape[1], up.shape[1]))
    table = ops.LoraJobTable(recs, dev)
    rec = table.host[::-1].copy()
    devrec = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    assert lib.sidlsg_lora_merge_f32.raw(rec.ctypes.data, devrec.data_ptr(), 2, table.nblocks, torch.cuda.current_stream().cuda_stream) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((t[1] == -3.0).all()) for t in keep)
    # Python names the layer
    bad = table.host.copy()
    bad['R'][1] = 6
    table.host = bad
    with pytest.raises(ValueError, match='second.layer'):
        ops.lora_merge(table, ['first.layer', 'second.layer'])


# ---- bookkeeping on random:tiny -------------------------------------------------------------------------------------------------------
TINY_TE = dict(hidden=64, layers=2, heads=2, dff=128, max_pos=13, act='quick_gelu')
_cache = {}


def tiny_state(name='tiny'):
    """(diffusers-layout UNet state dict, text encoder state dict) of the seeded model, CPU fp32, built once."""
    from sid_lsg_amd.text import CLIPTextModel
    from sid_lsg_amd.unet import CONFIGS, random_state_dict
    if name not in _cache:
        torch.manual_seed(1)
        te = CLIPTextModel(**TINY_TE).requires_grad_(False).eval()
        _cache[name] = (random_state_dict(CONFIGS[name], 0), {k: v.clone() for k, v in te.state_dict().items()})
    return _cache[name]


def make_unet(name, cd, dev, source=None):
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    usd = tiny_state(name)[0] if source is None else source
    return HipUNet2DCondition(CONFIGS[name], compute_dtype=cd).materialize(dev, with_grad_buffers=False, source=usd).requires_grad_(False).eval()


def make_te(dev, state=None, hip=False):
    from sid_lsg_amd.text import CLIPTextModel, HipCLIPTextModel
    te = CLIPTextModel(**TINY_TE).requires_grad_(False).eval()
    te.load_state_dict(tiny_state()[1] if state is None else state)
    te = te.to(dev)
    return HipCLIPTextModel.from_torch(te) if hip else te


def lora_file(name, rank, seed):
    """(kohya state dict, its adapters for the unmaterialised networks) of random:lora at `rank` / `seed`, built once."""
    from sid_lsg_amd import lora
    from sid_lsg_amd.text import CLIPTextModel
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    key = ('file', name, rank, seed)
    if key not in _cache:
        usd, tsd = tiny_state(name)
        te = CLIPTextModel(**TINY_TE)
        te.load_state_dict(tsd)
        meta = HipUNet2DCondition(CONFIGS[name])
        sd = lora.random_lora_state_dict(meta, te, rank, seed, unet_state=usd)
        _cache[key] = (sd, lora.parse_lora(sd, meta, te))
    return _cache[key]


def merged_ref(name, files, scales):
    """The fp64 merged state dicts, rounded to fp32 (what a fresh network loads), and the per-element bound magnitudes are not needed
    here: the bookkeeping test compares the fresh network's masters under the float-case bound."""
    usd, tsd = tiny_state(name)
    mu, mt = lora_ref.merge(usd, tsd, files, scales)
    return {k: v.float() for k, v in mu.items()}, {k: v.float() for k, v in mt.items()}, mu, mt


def master_bound(name, files, scales, rpad, net='unet'):
    """Per weight of `net` the float-case bound (R + 3) 2^-24 (|W| + sum |coef up down|) in the state dict's layout, R the padded
    concatenated rank.  Every coefficient scale * alpha / rank used with it (1, 0.5, 0.75, -0.5; alpha = rank) is exact in fp32, so the
    kernel's fp32 coefficient is the reference's fp64 one and the bound has no term for it."""
    usd, tsd = tiny_state(name)
    src = usd if net == 'unet' else tsd
    out = {}
    for sd, s in zip(files, scales):
        for (n, mod), p in lora_ref.walk(sd, usd, tsd).items():
            if n != net:
                continue
            rank = p['down'].shape[0]
            alpha = float(p['alpha']) if 'alpha' in p else float(rank)
            mag = lora_ref.delta(src[mod + '.weight'], p['down'].abs(), p['up'].abs(), alpha) * abs(float(s))
            out[mod] = out.get(mod, src[mod + '.weight'].double().abs()) + mag
    return {mod: (rpad + 3) * U * m for mod, m in out.items()}


def check_masters(net_obj, name, files, scales, rpad, what, net='unet'):
    """The masters of `net_obj` against the fp64 merge under the bound; keys that are no target must not have changed at all."""
    f32u, f32t, mu, mt = merged_ref(name, files, scales)
    ref_sd, base_sd = (mu, tiny_state(name)[0]) if net == 'unet' else (mt, tiny_state(name)[1])
    bound = master_bound(name, files, scales, rpad, net)
    got = {k: v.detach().cpu().double() for k, v in net_obj.state_dict().items()}
    worst = 0.0
    assert len(bound) > 10
    for k, ref in ref_sd.items():
        mod = k[:-len('.weight')] if k.endswith('.weight') else None
        if mod in bound:
            ratio = float(((got[k] - ref).abs() / bound[mod]).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f'{what}: {k}: {ratio:.3f} x the bound'
            assert float((ref - base_sd[k].double()).norm()) > 0.05 * float(ref.norm()), f'{k}: the adapter does not move this weight'
        else:
            assert torch.equal(got[k], base_sd[k].double()), f'{what}: {k} is not a target and must not change'
    return worst, (f32u if net == 'unet' else f32t)


def w16(unet):
    """The flat compute copy of the weights: the bf16 buffer, or (fp32 mode) the masters themselves."""
    return unet._flat['w16']


def q_rows(unet):
    """The pre-scaled q rows of w16 (bf16 mode), concatenated."""
    from sid_lsg_amd.unet import Attention
    fl = unet._flat
    parts = []
    for n, m in unet.named_modules():
        if isinstance(m, Attention):
            o = fl['offs'][f'{n}.to_q.weight']
            parts.append(fl['w16'][o:o + m.to_q.weight.numel()])
    return torch.cat(parts)


@pytest.mark.parametrize('cd', [F32, BF16], ids=['fp32', 'bf16'])
def test_attach_set_scales_detach_on_tiny(dev, cd):
    from sid_lsg_amd import lora
    name = 'tiny'
    sd, ad = lora_file(name, 4, 0)
    unet, te = make_unet(name, cd, dev), make_te(dev)
    p0, w0, te0 = unet.flat_params.clone(), w16(unet).clone(), {k: v.clone() for k, v in te.state_dict().items()}
    ls = lora.LoraSet(unet, te).attach([ad], [1.0])
    worst, f32sd = check_masters(unet, name, [sd], [1.0], 4, 'attach at 1')
    print(f'tiny {cd}: masters after attach, worst |got - fp64| / bound = {worst:.4f}')
    assert not torch.equal(unet.flat_params, p0)
    # compute copies: bit-equal to those of a fresh network given the attached masters
    fresh = make_unet(name, cd, dev, source=f32sd)
    fresh.flat_params.copy_(unet.flat_params)
    fresh.refresh_compute_weights()
    assert torch.equal(w16(fresh), w16(unet))
    if cd == BF16:
        assert unet._flat['w16_prescaled'] and torch.equal(q_rows(fresh), q_rows(unet))
    # text encoder masters against the reference
    worst_te, _ = check_masters(te, name, [sd], [1.0], 4, 'attach at 1 (text encoder)', net='te')
    print(f'tiny {cd}: text-encoder masters after attach, worst |got - fp64| / bound = {worst_te:.4f}')
    # set_scales([0.5]) == a fresh attach at 0.5, bit for bit
    ls.set_scales([0.5])
    half = unet.flat_params.clone(), w16(unet).clone(), {k: v.clone() for k, v in te.state_dict().items()}
    u2, t2 = make_unet(name, cd, dev), make_te(dev)
    lora.LoraSet(u2, t2).attach([ad], [0.5])
    assert torch.equal(u2.flat_params, half[0]) and torch.equal(w16(u2), half[1])
    assert all(torch.equal(v, half[2][k]) for k, v in t2.state_dict().items())
    check_masters(unet, name, [sd], [0.5], 4, 'set_scales 0.5')
    # all zeros, then detach: the original masters and compute copies
    ls.set_scales([0.0])
    assert torch.equal(unet.flat_params, p0) and torch.equal(w16(unet), w0)
    assert all(torch.equal(v, te0[k]) for k, v in te.state_dict().items())
    ls.set_scales([-1.0])
    assert not torch.equal(unet.flat_params, p0)
    ls.detach()
    assert torch.equal(unet.flat_params, p0) and torch.equal(w16(unet), w0) and not ls.attached
    assert all(torch.equal(v, te0[k]) for k, v in te.state_dict().items())
    with pytest.raises(RuntimeError, match='nothing attached'):
        ls.set_scales([1.0])


def test_two_adapters_equal_the_reference_of_their_sum_and_fuse_equals_attach(dev):
    from sid_lsg_amd import lora
    name = 'tiny'
    (sd_a, ad_a), (sd_b, ad_b) = lora_file(name, 4, 0), lora_file(name, 6, 9)
    unet, te = make_unet(name, F32, dev), make_te(dev)
    ls = lora.LoraSet(unet, te).attach([ad_a, ad_b], [0.75, -0.5])
    worst, _ = check_masters(unet, name, [sd_a, sd_b], [0.75, -0.5], 12, 'two adapters')          # 4 + 6 = 10 columns, padded to 12
    print(f'tiny fp32: two adapters (ranks 4 + 6), worst |got - fp64| / bound = {worst:.4f}')
    u2, t2 = make_unet(name, F32, dev), make_te(dev)
    lora.fuse(u2, t2, [ad_a, ad_b], [0.75, -0.5])
    assert torch.equal(u2.flat_params, unet.flat_params) and torch.equal(w16(u2), w16(unet))
    assert all(torch.equal(v, te.state_dict()[k]) for k, v in t2.state_dict().items())
    # fusing is allowed on a network that trains
    u3 = make_unet(name, BF16, dev).requires_grad_(True)
    lora.fuse(u3, None, [[e for e in ad_a if e[0][0] == 'unet']], [1.0])
    assert not torch.equal(u3.flat_params, make_unet(name, BF16, dev).flat_params)


# ---- the adapted networks -------------------------------------------------------------------------------------------------------------
def unet_inputs(cfg, B=2, lat=8, seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, lat, lat, generator=g)
    t = torch.tensor([500, 37][:B])
    ctx = torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g).to(BF16).float()
    return x, t, ctx


def run_unet(unet, x, t, ctx, dev):
    B, C, h, w = x.shape
    xin = torch.zeros(B, h, w, 8)
    xin[..., :C] = x.permute(0, 2, 3, 1)
    with torch.no_grad():
        eps = unet.forward_nhwc(xin.to(unet.compute_dtype).to(dev), t.to(dev), ctx.to(unet.compute_dtype).to(dev).contiguous())
    return eps.view(B, h, w, 8)[..., :4].permute(0, 3, 1, 2).float().cpu()


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def unet_only(ad):
    return [e for e in ad if e[0][0] == 'unet']


def test_unet_output_fp32_against_the_fresh_merged_network(dev):
    from sid_lsg_amd import lora
    from sid_lsg_amd.unet import CONFIGS
    name = 'tiny'
    sd, ad = lora_file(name, 4, 0)
    x, t, ctx = unet_inputs(CONFIGS[name])
    unet = make_unet(name, F32, dev)
    plain = run_unet(unet, x, t, ctx, dev)
    lora.LoraSet(unet).attach([unet_only(ad)], [1.0])
    got = run_unet(unet, x, t, ctx, dev)
    f32sd = merged_ref(name, [sd], [1.0])[0]
    want = run_unet(make_unet(name, F32, dev, source=f32sd), x, t, ctx, dev)
    err = float((got - want).abs().max()) / float(want.abs().max())
    moved = rel_l2(got, plain)
    print(f'tiny fp32: attached UNet against the fresh merged network: max-norm error {err:.2e} (bound {FP32_TOL:g}); the adapter moves the output '
          f'by {moved:.3f} relative l2')
    assert torch.isfinite(got).all() and err <= FP32_TOL
    assert moved >= 100 * FP32_TOL


@pytest.mark.parametrize('name', ['tiny40', 'tiny21'])
def test_unet_output_bf16_error_is_at_most_twice_the_plain_error(dev, name):
    """Relative l2 of the bf16 attached output against the fp32 fresh merged network <= 2 x that of the plain bf16 UNet against the plain
    fp32 one (the rule of the ControlNet and IP-Adapter tests).  Both figures are printed (-s).  Measured on an MI355X (profiles/lora.txt):
    tiny40 plain 1.102e-2, attached 1.092e-2 (0.99 x); tiny21 plain 1.135e-2, attached 1.063e-2 (0.94 x)."""
    from sid_lsg_amd import lora
    from sid_lsg_amd.unet import CONFIGS
    sd, ad = lora_file(name, 4, 0)
    x, t, ctx = unet_inputs(CONFIGS[name])
    ref_plain = run_unet(make_unet(name, F32, dev), x, t, ctx, dev)
    ref_lora = run_unet(make_unet(name, F32, dev, source=merged_ref(name, [sd], [1.0])[0]), x, t, ctx, dev)
    unet = make_unet(name, BF16, dev)
    e_plain = rel_l2(run_unet(unet, x, t, ctx, dev), ref_plain)
    lora.LoraSet(unet).attach([unet_only(ad)], [1.0])
    got = run_unet(unet, x, t, ctx, dev)
    e_lora = rel_l2(got, ref_lora)
    print(f'{name} bf16: plain UNet rel l2 {e_plain:.3e}, with the LoRA attached {e_lora:.3e}, ratio {e_lora / e_plain:.2f}; '
          f'adapter effect {rel_l2(ref_lora, ref_plain):.3f}')
    assert torch.isfinite(got).all() and e_plain > 0 and rel_l2(ref_lora, ref_plain) > 0.01
    assert e_lora <= 2 * e_plain


@pytest.mark.parametrize('hip', [False, True], ids=['torch', 'hip'])
def test_text_encoder_fp32(dev, hip):
    """The module over the merged parameters against the module loaded from the reference's merged state dict, fp64 on the CPU; bound:
    2 x the error of the torch module on the device over the reference's own (fp32-rounded) merged weights -- the rule of
    tests/test_gpu_text_hip.py::test_encoder_matches_the_torch_module.  On the hip module the cache is rebuilt after attach, set_scales
    and detach."""
    from sid_lsg_amd import lora
    from sid_lsg_amd.text import CLIPTextModel, HashTokenizer
    name = 'tiny'
    sd, ad = lora_file(name, 4, 0)
    ids = HashTokenizer(model_max_length=13)(['', 'a red cube', 'word ' * 30]).input_ids
    _, f32te, _, mt = merged_ref(name, [sd], [1.0])
    ref = CLIPTextModel(**TINY_TE).double().requires_grad_(False).eval()
    ref.load_state_dict(mt)
    with torch.no_grad():
        want = ref(ids)[0]
        base = make_te(dev, state=f32te)(ids.to(dev))[0]
    unet, te = make_unet(name, F32, dev), make_te(dev, hip=hip)
    with torch.no_grad():
        before = te(ids.to(dev))[0].clone()
    cache0 = te._hip_cache if hip else None
    ls = lora.LoraSet(unet, te).attach([ad], [1.0])
    assert not hip or te._hip_cache is None
    with torch.no_grad():
        got = te(ids.to(dev))[0]
    rl = lambda a, b: float(((a.double().cpu() - b).flatten(1).norm(dim=1) / b.flatten(1).norm(dim=1)).max())      # noqa: E731
    e_got, e_base = rl(got, want), rl(base, want)
    print(f'text encoder ({"hip" if hip else "torch"}) fp32 with the LoRA: rel l2 against fp64 {e_got:.3e}; torch module over the reference weights {e_base:.3e}')
    assert e_got <= 2 * e_base and rl(before, want) > 0.01
    if hip:
        c1 = te._hip_cache
        assert c1 is not None and c1 is not cache0
        ls.set_scales([0.5])
        assert te._hip_cache is None
        with torch.no_grad():
            half = te(ids.to(dev))[0]
        assert te._hip_cache is not None and not torch.equal(half, got)
        ls.detach()
        assert te._hip_cache is None
    else:
        ls.detach()
    with torch.no_grad():
        assert torch.equal(te(ids.to(dev))[0], before)


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
def test_a_pass_with_an_adapter_issues_the_same_library_calls(dev, cd):
    from sid_lsg_amd import lora
    from sid_lsg_amd.unet import CONFIGS
    name = 'tiny'
    _, ad = lora_file(name, 4, 0)
    x, t, ctx = unet_inputs(CONFIGS[name])
    unet = make_unet(name, cd, dev)
    run_unet(unet, x, t, ctx, dev)
    with _CallCounter() as n_plain:
        plain = run_unet(unet, x, t, ctx, dev)
    ls = lora.LoraSet(unet).attach([unet_only(ad)], [1.0])
    run_unet(unet, x, t, ctx, dev)
    with _CallCounter() as n_lora:
        got = run_unet(unet, x, t, ctx, dev)
    assert n_lora == n_plain and sum(n_plain.values()) > 50 and n_lora['sidlsg_lora_merge_f32'] == 0
    assert not torch.equal(got, plain)
    ls.set_scales([0.0])
    assert torch.equal(run_unet(unet, x, t, ctx, dev), plain)


def test_refusals_on_the_gpu(dev):
    from sid_lsg_amd import lora, ops
    from sid_lsg_amd.controlnet import HipControlNet
    from sid_lsg_amd.unet import CONFIGS
    name = 'tiny'
    _, ad = lora_file(name, 4, 0)
    ad = unet_only(ad)
    unet = make_unet(name, BF16, dev)
    with pytest.raises(RuntimeError, match='requires_grad'):
        lora.LoraSet(make_unet(name, BF16, dev).requires_grad_(True)).attach([ad], [1.0])
    cn = HipControlNet(CONFIGS[name]).materialize(dev, seed=0)
    with pytest.raises(TypeError, match='ControlNet'):
        lora.LoraSet(cn)
    with pytest.raises(TypeError, match='ControlNet'):
        lora.fuse(cn, None, [ad], [1.0])
    q = make_unet(name, BF16, dev)
    q.enable_fp8_weights()
    with pytest.raises(RuntimeError, match='e4m3'):
        lora.LoraSet(q).attach([ad], [1.0])
    ls = lora.LoraSet(unet).attach([ad], [1.0])
    with pytest.raises(RuntimeError, match='already attached'):
        ls.attach([ad], [1.0])
    other = make_unet(name, BF16, dev)
    with ops.dual_networks(unet.partner_map(other)):
        with pytest.raises(RuntimeError, match='grouped pass'):
            ls.set_scales([0.5])
    with pytest.raises(ValueError, match='one per file'):
        ls.set_scales([1.0, 2.0])
    ls.detach()
    with pytest.raises(ValueError, match='no text encoder'):
        lora.LoraSet(unet).attach([lora_file(name, 4, 0)[1]], [1.0])
    assert torch.equal(unet.flat_params, other.flat_params)


# ---- command lines --------------------------------------------------------------------------------------------------------------------
def _run(args, timeout=240):
    with socket.socket() as sock:           # a rendezvous port of the child's own: this process may hold the default one
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    res = subprocess.run([sys.executable] + args, cwd=ROOT, env=dict(os.environ, MASTER_PORT=str(port)), capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def _png_pixels(path):
    import PIL.Image
    return np.asarray(PIL.Image.open(path).convert('RGB'))


def test_generate_onestep_with_a_lora(dev, tmp_path):
    """`generate_onestep.py --network teacher --teacher_steps 2 --lora random:lora` in a child process; then, in this process, the plain run,
    the run at --lora_scale 0 and a run with two files and one scale: the LoRA changes the images, scale 0 gives the plain run's files
    byte for byte."""
    from click.testing import CliRunner

    import generate_onestep
    prompts = tmp_path / 'prompts.txt'
    prompts.write_text('a red cube\na blue sphere\n')
    common = ['--network', 'teacher', '--repo_id', 'random:tiny', '--teacher_steps', '2', '--seeds', '0-1', '--resolution', '64', '--text_prompts', str(prompts)]
    out_a, out_z, out_p, out_2 = (tmp_path / n for n in ('a', 'z', 'plain', 'two'))
    log = _run([os.path.join(ROOT, 'generate_onestep.py'), '--outdir', str(out_a)] + common + ['--lora', 'random:lora', '--text_encoder', 'hip'])
    assert 'LoRA "random:lora":' in log and 'rank 4, scale 1' in log and 'not comparable' in log, log
    r = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out_z)] + common + ['--lora', 'random:lora', '--lora_scale', '0', '--text_encoder', 'hip'],
                           catch_exceptions=False)
    assert r.exit_code == 0 and 'scale 0' in r.output, r.output
    r = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out_p)] + common + ['--text_encoder', 'hip'], catch_exceptions=False)
    assert r.exit_code == 0 and 'LoRA' not in r.output, r.output
    r = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out_2)] + common + ['--lora', 'random:lora', '--lora', 'random:lora:8:3', '--lora_scale', '-0.5'],
                           catch_exceptions=False)
    assert r.exit_code == 0 and 'rank 8, scale -0.5' in r.output and 'rank 4, scale -0.5' in r.output, r.output
    names = ['000000.png', '000001.png']
    for d in (out_a, out_z, out_p, out_2):
        assert [os.path.basename(f) for f in sorted(glob.glob(str(d / '*.png')))] == names
    for n in names:
        a, p = _png_pixels(str(out_a / n)), _png_pixels(str(out_p / n))
        assert a.shape == (64, 64, 3) and a.min() != a.max() and not np.array_equal(a, p)
        assert not np.array_equal(_png_pixels(str(out_2 / n)), p)
        assert open(out_z / n, 'rb').read() == open(out_p / n, 'rb').read()


def test_sid_train_with_a_lora(dev, tmp_path):
    """tests/lora_loop_worker.py runs the loop of `sid_train.py` for two iterations on random:tiny three times in one child process:
    without the option, with an empty LoRA list, with random:lora.  The first two give the same losses bit for bit (deterministic mode);
    the third starts all networks from the fused model: its snapshot lies within 3 lr of the reference's merged weights (two Adam steps
    with beta1 = 0 move a weight by at most (1 + sqrt(1 + beta2)) lr < 3 lr, and the EMA is a convex combination of the iterates) and
    far from the base model."""
    import pickle
    out = tmp_path / 'out.pt'
    _run([os.path.join(ROOT, 'tests', 'lora_loop_worker.py'), str(out), str(tmp_path)])
    res = torch.load(str(out), weights_only=False)
    assert len(res['none']['losses']) == 4 and torch.equal(res['none']['losses'], res['empty']['losses'])
    assert torch.equal(res['none']['G'], res['empty']['G'])
    assert not torch.equal(res['none']['losses'], res['lora']['losses'])
    with open(res['lora']['snapshot'], 'rb') as f:
        ema = pickle.load(f)['ema']
    from sid_lsg_amd.training_loop import _snapshot_state
    got = {k: v.detach().cpu().double() for k, v in _snapshot_state(ema).items()}
    sd, _ = lora_file('tiny', 4, 0)
    mu = merged_ref('tiny', [sd], [1.0])[2]
    lr = res['lr']
    base = tiny_state('tiny')[0]
    for k, ref in mu.items():
        assert float((got[k] - ref).abs().max()) <= 3 * lr + 8 * U * float(ref.abs().max()), k
    far = [k for k in mu if k.endswith('.weight') and mu[k].dim() in (2, 4)]
    assert len(far) > 200 and all(float((got[k] - base[k].double()).norm()) > 0.05 * float(base[k].double().norm()) for k in far)
    # the sid_train.py command line accepts the options
    from click.testing import CliRunner

    import sid_train
    r = CliRunner().invoke(sid_train.main, ['--outdir', str(tmp_path / 'runs'), '--data_prompt_text', str(tmp_path / 'prompts'), '--sd_model', 'random:tiny',
                                            '--seed', '3', '--batch', '8', '--batch-gpu', '2', '--duration', '0.01', '--dry-run', '--lora', 'random:lora'])
    assert r.exit_code == 0 and '"random:lora"' in r.output, r.output


def test_snapshot_evaluation_fuses_only_the_text_encoder(dev):
    """training_loop._fuse_lora(text_encoder_only=True), the `--train_mode 0` path of a snapshot: the text encoder ends up as after a
    full fuse, the UNet's masters and compute copies are untouched; a file without text-encoder layers changes nothing."""
    from sid_lsg_amd import lora
    from sid_lsg_amd import training_loop as tl
    name = 'tiny'
    _, ad = lora_file(name, 4, 0)
    unet, te = make_unet(name, BF16, dev), make_te(dev)
    p0, w0 = unet.flat_params.clone(), w16(unet).clone()
    tl._fuse_lora(dict(specs=['random:lora:4:0'], scales=[0.5]), unet, te, text_encoder_only=True)
    assert torch.equal(unet.flat_params, p0) and torch.equal(w16(unet), w0)
    u2, t2 = make_unet(name, BF16, dev), make_te(dev)
    lora.fuse(u2, t2, [ad], [0.5])
    assert all(torch.equal(v, t2.state_dict()[k]) for k, v in te.state_dict().items())
    assert not torch.equal(u2.flat_params, p0)
    assert any(not torch.equal(v, tiny_state(name)[1][k].to(dev)) for k, v in te.state_dict().items())
