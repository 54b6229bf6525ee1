"""The argument contract of the GEMM / conv / weight-gradient entry points of csrc/gemm.hip, gemm_fp8.hip and wgrad.hip, checked without a GPU.

Every entry point rejects a bad call with SIDLSG_EINVAL (-22) before its first HIP call.  For each one the table below holds one
admissible argument list and flips one thing at a time.  The calls run in a child process that sees no GPU (HIP_VISIBLE_DEVICES=-1),
so nothing is launched on any machine: an admitted call comes back with a HIP "no device" code, a rejected one with -22, and a
rejection that went missing shows up as the former.  The operands are addresses of a 16-byte-aligned host buffer: the entry points
never dereference them on the host (the `jobs` records of the grouped weight gradient are host memory by contract)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
LIMIT = 2 ** 31 - 1          # an operand extent must stay below this many bytes (31-bit buffer descriptors)
OUT_F32, SILU, ACCUM = 1, 2, 4
P = 'ptr'                    # placeholder: the worker puts the address of its buffer here


def _cases():
    """-> [(entry point, label, {argument: value}, rejected?)]: the admissible list first, then one flip each."""
    out = []

    def family(name, base, flips, admitted=()):
        out.append((name, 'admissible', dict(base), False))
        for label, over in admitted:
            out.append((name, label, {**base, **over}, False))
        for label, over in flips:
            out.append((name, label, {**base, **over}, True))

    def nulls(*names):
        return [(f'null {n}', {n: None}) for n in names]

    def nonpos(*names):
        return [(f'{n} = {v}', {n: v}) for n in names for v in (0, -8)]

    def contract(out, n, n_name, ld_in, k):
        """The operand contract of the output and the epilogue operands (include/sidlsg_hip.h "operand contract") for a family whose base has
        `n` % 8 == 0 output columns (argument `n_name`) in rows of ldc = n, and `k` input columns in rows of `ld_in`: -> (flips, admitted)."""
        flips = [(f'ldc < {n_name}', dict(ldc=n - 8)), (f'ldres < {n_name}', dict(res=P, ldres=n - 8)), (f'ld_rowvec < {n_name}', dict(rowvec=P, ld_rowvec=n - 8)),
                 (f'{ld_in} < its {k} columns', {ld_in: k - 8}),
                 (f'ldc % 8 with {n_name} % 8 == 0', dict(ldc=n + 4)), (f'fp32 {out} with ldc % 4', dict(ldc=n + 2, flags=OUT_F32)), (f'misaligned {out}', {out: 'ptr+8'}),
                 ('ldres % 8', dict(res=P, ldres=n + 4)), ('misaligned res', dict(res='ptr+8', ldres=n)),
                 ('ld_rowvec % 4', dict(rowvec=P, ld_rowvec=n + 2)), ('misaligned rowvec', dict(rowvec='ptr+8', ld_rowvec=n)), ('misaligned bias', dict(bias='ptr+8'))]
        admitted = [('wider ldc, ldres and ld_rowvec', dict(ldc=n + 8, res=P, ldres=n + 64, rowvec=P, ld_rowvec=n + 4)),
                    (f'fp32 {out} with ldc % 8 == 4', dict(ldc=n + 4, flags=OUT_F32)), ('ldres = N, ld_rowvec = 0 (= N)', dict(res=P, ldres=n, rowvec=P, ld_rowvec=0))]
        return flips, admitted

    def ragged(n_name, n):
        """N % 8 != 0 takes the element-wise epilogue: no alignment demands, the widths still hold."""
        return ([(f'ragged {n_name}: ldc < {n_name}', {n_name: n - 4, 'ldc': n - 8})],
                [(f'ragged {n_name}: odd strides, misaligned operands', {n_name: n - 4, 'ldc': n - 3, 'res': 'ptr+8', 'ldres': n - 1, 'rowvec': 'ptr+8', 'ld_rowvec': n - 2, 'bias': 'ptr+8'})])

    epi = dict(ldc=64, bias=P, res=None, ldres=0, rowvec=None, ld_rowvec=0, alpha=1.0, flags=0, stream=None)
    epi_flips = [('ACCUM without OUT_F32', dict(flags=ACCUM)), ('ACCUM | SILU without OUT_F32', dict(flags=ACCUM | SILU))]
    epi_ok = [('ACCUM with OUT_F32', dict(flags=ACCUM | OUT_F32))]

    # ---- dense, bf16 activations.  Extents: A ((M - 1) lda + K) * 2 bytes, W N * K * 2 (fp8w: N * K)
    for name, kq, g2 in (('sidlsg_gemm_bf16', 8, 0), ('sidlsg_gemm_bf16_g2', 8, 1), ('sidlsg_gemm_fp8w', 16, 0), ('sidlsg_gemm_fp8w_g2', 16, 1)):
        f8 = 'fp8w' in name
        w = 'W8' if f8 else 'W'
        base = dict(A=P, lda=64, C=P, rows_per_batch=1, M=64, N=64, K=64, **epi, **{w: P})
        flips = nulls('A', w, 'C') + nonpos('M', 'N', 'K') + epi_flips
        flips += [(f'K % {kq}', dict(K=64 + kq // 2)), ('lda % 8', dict(lda=68)),
                  ('rowvec with rows_per_batch = 0', dict(rowvec=P, rows_per_batch=0)), ('rowvec with rows_per_batch < 0', dict(rowvec=P, rows_per_batch=-1))]
        admitted = epi_ok + [('rowvec with rows_per_batch = 1', dict(rowvec=P))]
        # A: lda = 2^20 -> 2^21 bytes per row: 1024 rows stay below 2^31 - 1, 1025 do not
        a_big = dict(K=16, lda=1 << 20)
        assert (1023 * (1 << 20) + 16) * 2 < LIMIT <= (1024 * (1 << 20) + 16) * 2
        admitted.append(('A extent just below 2^31 - 1', dict(M=1024, **a_big)))
        flips.append(('A extent past 2^31 - 1', dict(M=1026, **a_big)))
        wk = 65536 if f8 else 32768          # one W row = 65536 bytes in both formats
        assert 32767 * 65536 < LIMIT <= 32768 * 65536
        admitted.append(('W extent just below 2^31 - 1', dict(M=2, N=32767, ldc=32767, K=wk, lda=wk)))
        flips.append(('W extent past 2^31 - 1', dict(M=2, N=32768, ldc=32768, K=wk, lda=wk)))
        for fl, ad in (contract('C', 64, 'N', 'lda', 64), ragged('N', 64)):
            flips += fl
            admitted += ad
        if f8:
            base['wscale'] = P
            flips += nulls('wscale')
        if g2:
            w1 = 'W8_1' if f8 else 'W1'
            base.update({w1: P, 'bias1': P})
            flips += nulls(w1) + [('odd M', dict(M=63)), ('bias for the first set only', dict(bias1=None)), ('bias for the second set only', dict(bias=None))]
            admitted.append(('no bias in either set', dict(bias=None, bias1=None)))
            if f8:
                base['wscale1'] = P
                flips += nulls('wscale1')
        family(name, base, flips, admitted)

    # ---- dense, e4m3 activations: extents in bytes of e4m3 (A (M - 1) lda + K, W N * K), so twice the element count of bf16
    for name, g2 in (('sidlsg_gemm_mx8', 0), ('sidlsg_gemm_mx8_g2', 1)):
        base = dict(A8=P, lda=64, W8=P, wscale=P, C=P, rows_per_batch=1, M=64, N=160, K=64, **epi)
        base['ldc'] = 160
        flips = nulls('A8', 'W8', 'wscale', 'C') + nonpos('M', 'N', 'K') + epi_flips
        flips += [('K % 16', dict(K=72, lda=80)), ('lda % 16', dict(lda=72)), ('lda < K', dict(lda=48)), ('N % 160', dict(N=128)), ('N % 160 (80)', dict(N=240)),
                  ('rowvec with rows_per_batch = 0', dict(rowvec=P, rows_per_batch=0))]
        admitted = epi_ok + [('rowvec with rows_per_batch = 1', dict(rowvec=P))]
        assert 2047 * (1 << 20) + 16 < LIMIT <= 2048 * (1 << 20) + 16
        admitted.append(('A extent just below 2^31 - 1', dict(M=2048, K=16, lda=1 << 20)))
        admitted.append(('A extent of 1026 rows (past the bf16 limit)', dict(M=1026, K=16, lda=1 << 20)))
        flips.append(('A extent past 2^31 - 1', dict(M=2050, K=16, lda=1 << 20)))
        k_ok, k_bad = 13421760, 13421776
        assert k_ok % 16 == 0 and k_bad % 16 == 0 and 160 * k_ok < LIMIT <= 160 * k_bad
        admitted.append(('W extent just below 2^31 - 1', dict(M=2, K=k_ok, lda=k_ok)))
        flips.append(('W extent past 2^31 - 1', dict(M=2, K=k_bad, lda=k_bad)))
        fl, ad = contract('C', 160, 'N', 'lda', 64)
        flips += [f for f in fl if not f[0].startswith('lda <')]          # ('lda < K' above: 48 is also lda % 16 == 0)
        admitted += ad
        if g2:
            base.update(W8_1=P, wscale1=P, bias1=P)
            flips += nulls('W8_1', 'wscale1') + [('odd M', dict(M=63)), ('bias for the first set only', dict(bias1=None)),
                                                 ('bias for the second set only', dict(bias=None))]
        family(name, base, flips, admitted)

    # ---- 3x3 convolutions.  Extent of the image: ((B Hs Ws - 1) ldx + Cin) elements, Hs x Ws = the SOURCE (half of H x Wd under `ups`)
    geo = dict(B=2, H=8, Wd=8, Cin=64, Cout=64, stride=1, ups=0)
    ldx_ok, ldx_bad = 1025 * 1024, 1025 * 1024 + 8        # 1024 source pixels
    assert (1023 * ldx_ok + 8) * 2 < LIMIT <= (1023 * ldx_bad + 8) * 2
    co_ok, co_bad = 3640, 3641                             # weight rows of 9 * 32768 elements
    assert co_ok * 9 * 32768 * 2 < LIMIT <= co_bad * 9 * 32768 * 2
    for name, cq, g2 in (('sidlsg_conv3x3_bf16', 8, 0), ('sidlsg_conv3x3_bf16_g2', 8, 1), ('sidlsg_conv3x3_fp8w', 16, 0), ('sidlsg_conv3x3_fp8w_g2', 16, 1)):
        f8 = 'fp8w' in name
        w = 'W8' if f8 else 'W'
        base = dict(X=P, ldx=64, Y=P, **geo, **epi, **{w: P})
        flips = nulls('X', w, 'Y') + nonpos('B') + epi_flips
        flips += [('stride 3', dict(stride=3)), ('stride 0', dict(stride=0)), (f'Cin % {cq}', dict(Cin=64 + cq // 2, ldx=128)), ('ldx % 8', dict(ldx=68)),
                  ('ups with odd H', dict(ups=1, H=9)), ('ups with odd Wd', dict(ups=1, Wd=9))]
        admitted = epi_ok + [('stride 2', dict(stride=2)), ('ups with even H and Wd', dict(ups=1)), ('odd H and Wd without ups', dict(H=9, Wd=9))]
        big = dict(B=2, Cin=cq, Cout=8)          # 2 x 32 x 16 = 1024 source pixels
        assert (1023 * ldx_ok + cq) * 2 < LIMIT
        admitted.append(('image extent just below 2^31 - 1', dict(H=32, Wd=16, ldx=ldx_ok, **big)))
        flips.append(('image extent past 2^31 - 1', dict(H=32, Wd=16, ldx=ldx_bad, **big)))
        admitted.append(('ups: the source image (half size) just below 2^31 - 1', dict(H=64, Wd=32, ups=1, ldx=ldx_ok, **big)))
        flips.append(('ups: the source image past 2^31 - 1', dict(H=64, Wd=32, ups=1, ldx=ldx_bad, **big)))
        for fl, ad in (contract('Y', 64, 'Cout', 'ldx', 64), ragged('Cout', 64)):
            flips += fl
            admitted += ad
        if f8:                               # e4m3 weights: one byte each, so twice the rows fit
            assert 2 * co_ok * 9 * 32768 < LIMIT <= (2 * co_ok + 2) * 9 * 32768
            admitted.append(('W extent just below 2^31 - 1', dict(B=2, H=2, Wd=2, Cin=32768, ldx=32768, Cout=2 * co_ok, ldc=2 * co_ok)))
            flips.append(('W extent past 2^31 - 1', dict(B=2, H=2, Wd=2, Cin=32768, ldx=32768, Cout=2 * co_ok + 2, ldc=2 * co_ok + 8)))
            base['wscale'] = P
            flips += nulls('wscale')
        else:
            admitted.append(('W extent just below 2^31 - 1', dict(B=2, H=2, Wd=2, Cin=32768, ldx=32768, Cout=co_ok, ldc=co_ok)))
            flips.append(('W extent past 2^31 - 1', dict(B=2, H=2, Wd=2, Cin=32768, ldx=32768, Cout=co_bad, ldc=co_bad + 7)))
        if g2:
            w1 = 'W8_1' if f8 else 'W1'
            base.update({w1: P, 'bias1': P})
            flips += nulls(w1) + [('odd B', dict(B=3)), ('bias for the first set only', dict(bias1=None)), ('bias for the second set only', dict(bias=None))]
            if f8:
                base['wscale1'] = P
                flips += nulls('wscale1')
        family(name, base, flips, admitted)

    # e4m3 image: pad 1, stride 1, no upsampling; the range check counts the (Wd + 1) ldx halo of the tap offsets
    lh_ok, lh_bad = 2064880, 2064896                      # 2 x 32 x 16 = 1024 pixels, halo of 17
    assert lh_ok % 16 == 0 and lh_bad % 16 == 0 and (1023 + 17) * lh_ok + 16 < LIMIT <= (1023 + 17) * lh_bad + 16 and 1023 * lh_bad + 16 < LIMIT
    for name, g2 in (('sidlsg_conv3x3_mx8', 0), ('sidlsg_conv3x3_mx8_g2', 1)):
        base = dict(X8=P, ldx=64, W8=P, wscale=P, Y=P, B=2, H=8, Wd=8, Cin=64, Cout=160, **epi)
        base['ldc'] = 160
        flips = nulls('X8', 'W8', 'wscale', 'Y') + nonpos('B', 'H', 'Wd', 'Cin', 'Cout') + epi_flips
        flips += [('Cin % 16', dict(Cin=72, ldx=80)), ('ldx % 16', dict(ldx=72)), ('ldx < Cin', dict(ldx=48)), ('Cout % 160', dict(Cout=128)),
                  ('image extent + halo past 2^31 - 1', dict(H=32, Wd=16, Cin=16, ldx=lh_bad)),
                  ('W extent past 2^31 - 1', dict(Cin=32768, ldx=32768, H=2, Wd=2, Cout=7360, ldc=7360))]
        assert 7200 * 9 * 32768 < LIMIT <= 7360 * 9 * 32768
        admitted = epi_ok + [('image extent + halo just below 2^31 - 1', dict(H=32, Wd=16, Cin=16, ldx=lh_ok)),
                             ('W extent just below 2^31 - 1', dict(Cin=32768, ldx=32768, H=2, Wd=2, Cout=7200, ldc=7200))]
        fl, ad = contract('Y', 160, 'Cout', 'ldx', 64)
        flips += [f for f in fl if not f[0].startswith('ldx <')]          # ('ldx < Cin' above)
        admitted += ad
        if g2:
            base.update(W8_1=P, wscale1=P, bias1=P)
            flips += nulls('W8_1', 'wscale1') + [('odd B', dict(B=3)), ('bias for the first set only', dict(bias1=None)),
                                                 ('bias for the second set only', dict(bias=None))]
        family(name, base, flips, admitted)

    # the down-sampling conv of the VAE encoder: its own admission rule
    base = dict(X=P, ldx=64, W=P, Y=P, ldc=64, bias=P, B=2, H=8, Wd=8, Cin=64, Cout=64, flags=0, stream=None)
    flips = nulls('X', 'W', 'Y') + nonpos('B', 'H', 'Wd') + [
        ('odd H', dict(H=9)), ('odd Wd', dict(Wd=9)), ('Cin % 8', dict(Cin=68, ldx=128)), ('ldx % 8', dict(ldx=68)), ('ldx < Cin', dict(ldx=56)), ('ldc < Cout', dict(ldc=56)),
        ('flag ACCUM', dict(flags=ACCUM | OUT_F32)), ('flag bit 3', dict(flags=8)),
        ('image extent past 2^31 - 1', dict(B=1, H=32, Wd=32, Cin=8, Cout=8, ldx=ldx_bad)),
        ('W extent past 2^31 - 1', dict(H=2, Wd=2, Cin=32768, ldx=32768, Cout=co_bad, ldc=co_bad))]
    admitted = [('OUT_F32 | SILU', dict(flags=OUT_F32 | SILU)), ('no bias', dict(bias=None)),
                ('image extent just below 2^31 - 1', dict(B=1, H=32, Wd=32, Cin=8, Cout=8, ldx=ldx_ok)),
                ('W extent just below 2^31 - 1', dict(H=2, Wd=2, Cin=32768, ldx=32768, Cout=co_ok, ldc=co_ok))]
    family('sidlsg_conv3x3_br_bf16', base, flips, admitted)

    # ---- GEGLU fusions: admitted from 256 tiles of 128 x 160 on
    la_ok, la_bad = 65536, 65544
    assert (16383 * la_ok + 8) * 2 < LIMIT <= (16383 * la_bad + 8) * 2
    kw_ok, kw_bad = 3355440, 3355448
    assert kw_ok % 8 == 0 and kw_bad % 8 == 0 and 320 * kw_ok * 2 < LIMIT <= 320 * kw_bad * 2
    for name, g2 in (('sidlsg_gemm_geglu_bf16', 0), ('sidlsg_gemm_geglu_bf16_g2', 1)):
        base = dict(A=P, lda=64, W=P, H=P, ldh=320, Y=P, ldy=160, bias=P, M=16384, N2=320, K=64, stream=None)
        flips = nulls('A', 'W', 'Y') + nonpos('M', 'N2', 'K') + [
            ('N2 % 160', dict(N2=384)), ('N2 % 160 (80)', dict(N2=400)), ('K % 8', dict(K=68)), ('too few tiles', dict(M=16256)), ('lda % 8', dict(lda=68)),
            ('ldh % 8', dict(ldh=324)), ('ldy % 8', dict(ldy=164)), ('A extent past 2^31 - 1', dict(K=8, lda=la_bad)), ('W extent past 2^31 - 1', dict(K=kw_bad, lda=8))]
        admitted = [('h not stored', dict(H=None)), ('no bias', dict(bias=None) if not g2 else dict(bias=None, bias1=None)),
                    ('A extent just below 2^31 - 1', dict(K=8, lda=la_ok)), ('W extent just below 2^31 - 1', dict(K=kw_ok, lda=8))]
        if g2:
            base.update(W1=P, bias1=P)
            flips += nulls('W1') + [('odd M', dict(M=16385)), ('bias for the first set only', dict(bias1=None)), ('bias for the second set only', dict(bias=None))]
        family(name, base, flips, admitted)
    kf_ok, kf_bad = 6710880, 6710888
    assert kf_ok % 8 == 0 and kf_bad % 8 == 0 and 160 * kf_ok * 2 < LIMIT <= 160 * kf_bad * 2
    lb_ok, lb_bad = 32768, 32776
    assert (32767 * lb_ok + 8) * 2 < LIMIT <= (32767 * lb_bad + 8) * 2
    for name, g2 in (('sidlsg_gemm_geglu_bwd_bf16', 0), ('sidlsg_gemm_geglu_bwd_bf16_g2', 1)):
        base = dict(dOut=P, lda=64, Wt=P, H=P, dH=P, ldh=320, M=32768, F=160, K=64, stream=None)
        flips = nulls('dOut', 'Wt', 'H', 'dH') + nonpos('M', 'F', 'K') + [
            ('F % 160', dict(F=128, ldh=256)), ('F % 160 (80)', dict(F=240, ldh=480)), ('K % 8', dict(K=68)), ('too few tiles', dict(M=32640)), ('lda % 8', dict(lda=68)),
            ('ldh % 8', dict(ldh=324)), ('ldh < 2 F', dict(ldh=312)), ('ldh = F', dict(ldh=160)),
            ('A extent past 2^31 - 1', dict(K=8, lda=lb_bad)), ('W extent past 2^31 - 1', dict(K=kf_bad, lda=8))]
        admitted = [('wider ldh', dict(ldh=328)), ('A extent just below 2^31 - 1', dict(K=8, lda=lb_ok)), ('W extent just below 2^31 - 1', dict(K=kf_ok, lda=8))]
        if g2:
            base.update(Wt1=P)
            flips += nulls('Wt1') + [('odd M', dict(M=32769))]
        family(name, base, flips, admitted)

    # ---- weight gradients.  Extents: A as above, dY ((M - 1) ldy + N) * 2 bytes
    for name in ('sidlsg_wgrad_bf16', 'sidlsg_wgrad_assign_bf16'):
        base = dict(dY=P, ldy=64, A=P, lda=64, dW=P, dBias=P, M=256, N=64, K=64, stream=None)
        flips = nulls('dY', 'A', 'dW') + nonpos('M', 'N', 'K') + [
            ('K % 8', dict(K=68)), ('lda % 8', dict(lda=68)), ('A extent past 2^31 - 1', dict(M=1026, K=16, lda=1 << 20)),
            ('dY extent past 2^31 - 1', dict(M=1026, N=16, ldy=1 << 20))]
        admitted = [('no bias gradient', dict(dBias=None)), ('A extent just below 2^31 - 1', dict(M=1024, K=16, lda=1 << 20)),
                    ('dY extent just below 2^31 - 1', dict(M=1024, N=16, ldy=1 << 20))]
        family(name, base, flips, admitted)
    for name in ('sidlsg_conv3x3_wgrad_bf16', 'sidlsg_conv3x3_wgrad_assign_bf16'):
        base = dict(dY=P, ldy=64, X=P, ldx=64, dW=P, dBias=P, **geo, stream=None)
        flips = nulls('dY', 'X', 'dW') + [
            ('stride 3', dict(stride=3)), ('stride 0', dict(stride=0)), ('Cin % 8', dict(Cin=68, ldx=128)), ('ldx % 8', dict(ldx=68)),
            ('image extent past 2^31 - 1', dict(B=1, H=32, Wd=32, Cin=8, Cout=8, ldx=ldx_bad)),
            ('ups: the source image past 2^31 - 1', dict(B=1, H=64, Wd=64, ups=1, Cin=8, Cout=8, ldx=ldx_bad)),
            ('dY extent past 2^31 - 1', dict(B=1, H=32, Wd=32, Cin=8, Cout=8, ldy=ldx_bad))]
        admitted = [('stride 2', dict(stride=2)), ('no bias gradient', dict(dBias=None)),
                    ('image extent just below 2^31 - 1', dict(B=1, H=32, Wd=32, Cin=8, Cout=8, ldx=ldx_ok)),
                    ('ups: the source image just below 2^31 - 1', dict(B=1, H=64, Wd=64, ups=1, Cin=8, Cout=8, ldx=ldx_ok)),
                    ('dY extent just below 2^31 - 1', dict(B=1, H=32, Wd=32, Cin=8, Cout=8, ldy=ldx_ok))]
        family(name, base, flips, admitted)

    # grouped: `jobs` = list of job dicts, packed into the 64-byte records by the worker
    for name, q in (('sidlsg_wgrad_group_bf16', 64), ('sidlsg_wgrad_group160_bf16', 160)):
        job = dict(dY=P, A=P, dW=P, dBias=P, ldy=q, lda=q, M=256, N=q, K=q, assign=0)

        def jobs(n=3, **last):
            return dict(jobs=[dict(job) for _ in range(n - 1)] + [{**job, **last}], njobs=n)
        base = dict(**jobs(), stream=None)
        flips = [('null jobs', dict(jobs=None)), ('njobs = 0', dict(njobs=0)), ('njobs = -1', dict(njobs=-1)), ('njobs = 9', jobs(9)),
                 ('null dW in the last job', jobs(dW=None)), ('null dY in the last job', jobs(dY=None)), ('null A in the last job', jobs(A=None)),
                 ('M = 0 in the last job', jobs(M=0)), ('N = 0 in the last job', jobs(N=0)), ('K = 0 in the last job', jobs(K=0)),
                 ('N % 8 in the last job', jobs(N=q + 4)), ('K % 8 in the last job', jobs(K=q + 4)), ('lda % 8 in the last job', jobs(lda=q + 4)),
                 ('ldy % 8 in the last job', jobs(ldy=q + 4)), ('misaligned A in the last job', jobs(A='ptr+8')),
                 ('A extent past 2^31 - 1 in the last job', jobs(M=1026, lda=1 << 20)), ('dY extent past 2^31 - 1 in the last job', jobs(M=1026, ldy=1 << 20))]
        admitted = [('njobs = 8', jobs(8)), ('njobs = 1', jobs(1)), ('assign in the last job', jobs(assign=1)), ('no bias gradient in the last job', jobs(dBias=None))]
        if q == 160:
            flips += [('N % 160 in the last job', jobs(N=128)), ('K % 160 in the last job', jobs(K=240)), ('N % 160 in the first job', dict(jobs=[{**job, 'N': 128}, job, job]))]
        else:
            admitted += [('N = 128 in the last job', jobs(N=128))]
        family(name, base, flips, admitted)

    # ---- e4m3 conversions
    base = dict(src_bf16=P, dst_fp8=P, scale=P, rows=4, cols=64, stream=None)
    family('sidlsg_quantize_fp8_rows', base, nulls('src_bf16', 'dst_fp8', 'scale') + nonpos('rows', 'cols') + [('cols % 8', dict(cols=68))])
    base = dict(src_bf16=P, dst_fp8=P, n=4096, stream=None)
    family('sidlsg_cast_fp8', base, nulls('src_bf16', 'dst_fp8') + nonpos('n') + [('n % 8', dict(n=4100))])
    return out


# the two admission helpers answer 0 / 1: both sides of the 256-tile threshold, and the shape rules
OK_CASES = [('sidlsg_gemm_geglu_ok', (16384, 320, 64), 1), ('sidlsg_gemm_geglu_ok', (16257, 320, 64), 1), ('sidlsg_gemm_geglu_ok', (16256, 320, 64), 0),
            ('sidlsg_gemm_geglu_ok', (8192, 640, 64), 1), ('sidlsg_gemm_geglu_ok', (8064, 640, 64), 0), ('sidlsg_gemm_geglu_ok', (16384, 384, 64), 0),
            ('sidlsg_gemm_geglu_ok', (16384, 320, 68), 0), ('sidlsg_gemm_geglu_ok', (0, 320, 64), 0), ('sidlsg_gemm_geglu_ok', (16384, 320, 0), 0),
            ('sidlsg_gemm_geglu_bwd_ok', (32768, 160, 64), 1), ('sidlsg_gemm_geglu_bwd_ok', (32641, 160, 64), 1), ('sidlsg_gemm_geglu_bwd_ok', (32640, 160, 64), 0),
            ('sidlsg_gemm_geglu_bwd_ok', (16384, 320, 64), 1), ('sidlsg_gemm_geglu_bwd_ok', (16256, 320, 64), 0), ('sidlsg_gemm_geglu_bwd_ok', (32768, 240, 64), 0),
            ('sidlsg_gemm_geglu_bwd_ok', (32768, 160, 68), 0), ('sidlsg_gemm_geglu_bwd_ok', (32768, 0, 64), 0), ('sidlsg_gemm_geglu_bwd_ok', (-1, 160, 64), 0)]


def _arg_names():
    """-> {entry point: [argument names in order]} from the header."""
    from sid_lsg_amd._lib import HEADER
    src = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    return {m.group(1): [re.search(r'(\w+)$', a.strip()).group(1) for a in m.group(2).split(',')]
            for m in re.finditer(r'\bint\s+(sidlsg_\w+)\s*\(([^)]*)\)\s*;', src) if m.group(2).strip() not in ('', 'void')}


class _Job(ctypes.Structure):
    _fields_ = [('dY', ctypes.c_void_p), ('A', ctypes.c_void_p), ('dW', ctypes.c_void_p), ('dBias', ctypes.c_void_p), ('ldy', ctypes.c_int),
                ('lda', ctypes.c_int), ('M', ctypes.c_int), ('N', ctypes.c_int), ('K', ctypes.c_int), ('assign', ctypes.c_int), ('pad', ctypes.c_int * 2)]


def _worker():
    """Child process (no GPU visible): every call of the table -> its return code, as one JSON line."""
    assert os.environ.get('HIP_VISIBLE_DEVICES') == '-1'
    from sid_lsg_amd._lib import lib
    lib.load()
    names = _arg_names()
    raw = ctypes.create_string_buffer(4096 + 16)
    ptr = (ctypes.addressof(raw) + 15) & ~15
    keep = []

    def value(v):
        if v == P:
            return ptr
        if v == 'ptr+8':
            return ptr + 8
        if isinstance(v, list):
            arr = (_Job * len(v))()
            for rec, j in zip(arr, v):
                for k, x in j.items():
                    setattr(rec, k, value(x))
            keep.append(arr)
            return ctypes.addressof(arr)
        return v

    assert ctypes.sizeof(_Job) == 64
    codes = []
    for name, label, kw, _ in _cases():
        assert sorted(kw) == sorted(names[name]), (name, label, sorted(set(kw) ^ set(names[name])))
        codes.append(getattr(lib, name).raw(*[value(kw[a]) for a in names[name]]))
    oks = [getattr(lib, name).raw(*args) for name, args, _ in OK_CASES]
    print('RESULT ' + json.dumps(dict(codes=codes, oks=oks)))


@pytest.fixture(scope='module')
def results():
    env = {k: v for k, v in os.environ.items() if not k.startswith('SIDLSG_') or k == 'SIDLSG_LIB'}      # the knobs at their defaults
    env.update(HIP_VISIBLE_DEVICES='-1', PYTHONPATH=ROOT + os.pathsep + env.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


ENTRY_POINTS = list(dict.fromkeys(c[0] for c in _cases()))


def test_every_entry_point_is_in_the_table():
    want = ['sidlsg_gemm_bf16', 'sidlsg_conv3x3_bf16', 'sidlsg_gemm_geglu_bf16', 'sidlsg_gemm_geglu_bwd_bf16', 'sidlsg_gemm_fp8w', 'sidlsg_conv3x3_fp8w',
            'sidlsg_gemm_mx8', 'sidlsg_conv3x3_mx8']
    want += [n + '_g2' for n in want]
    want += ['sidlsg_conv3x3_br_bf16', 'sidlsg_wgrad_bf16', 'sidlsg_wgrad_assign_bf16', 'sidlsg_conv3x3_wgrad_bf16', 'sidlsg_conv3x3_wgrad_assign_bf16',
             'sidlsg_wgrad_group_bf16', 'sidlsg_wgrad_group160_bf16', 'sidlsg_quantize_fp8_rows', 'sidlsg_cast_fp8']
    assert sorted(want) == sorted(ENTRY_POINTS)


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_rejections_come_before_any_launch(results, name):
    cases = _cases()
    assert len(results['codes']) == len(cases)
    mine = [(label, rejected, rc) for (n, label, _, rejected), rc in zip(cases, results['codes']) if n == name]
    assert sum(r for _, r, _ in mine) >= 5 and not mine[0][1]
    wrong = [f'{label}: returned {rc}, expected {"-22" if rejected else "to be admitted"}' for label, rejected, rc in mine if (rc == EINVAL) != rejected]
    assert not wrong, name + ': ' + '; '.join(wrong)
    # an admitted call reaches HIP, which has no device here: nothing can have run
    assert all(rc != 0 for _, rejected, rc in mine if not rejected)


def test_geglu_admission_helpers(results):
    got = results['oks']
    wrong = [f'{name}{args} = {g}, expected {want}' for (name, args, want), g in zip(OK_CASES, got) if g != want]
    assert not wrong, '; '.join(wrong)


if __name__ == '__main__':
    _worker()
