#!/usr/bin/env python
"""Fused d = 40 attention backward (delta + attn_bwd_fused_kernel + slab reduce) against the two-kernel path (dQ + dK/dV), in one
process, at N 4096, d 40, 8 heads: time per call and rel-l2 difference of the gradients.  GPU only.
    python tools/ab/attn_bwd_fused.py [B ...]        (default 8 16 32)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from sid_lsg_amd import ops  # noqa: E402
from sid_lsg_amd._lib import lib  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
dev = torch.device('cuda:0')


def timeit(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def main():
    Bs = [int(a) for a in sys.argv[1:]] or [8, 16, 32]
    N, heads, D = 4096, 8, 40
    C = heads * D
    ops.ensure_workspace(dev)
    torch.manual_seed(0)
    s = torch.cuda.current_stream().cuda_stream
    old = lib.sidlsg_debug_set_attn_bwd_fused.raw(-1)
    for ps in (True, False):
        sfx = '_ps' if ps else ''
        for B in Bs:
            qkv = torch.randn(B, N, 3 * C, device=dev).to(BF16)
            if ps:
                qkv[..., :C] = (qkv[..., :C].float() * (D ** -0.5 * 1.4426950408889634)).to(BF16)
            do = torch.randn(B, N, C, device=dev).to(BF16)
            o = torch.empty(B, N, C, device=dev, dtype=BF16)
            lse = torch.empty(B, heads, N, device=dev, dtype=F32)
            delta = torch.empty(B, heads, N, device=dev, dtype=F32)
            q, k, v = (qkv.data_ptr() + 2 * C * i for i in range(3))
            getattr(lib, 'sidlsg_attn_fwd' + sfx)(q, k, v, o.data_ptr(), lse.data_ptr(), B, heads, N, N, D, 3 * C, 3 * C, 3 * C, C,
                                                  N * 3 * C, N * 3 * C, N * 3 * C, N * C, s)
            res = {}
            for mode in (0, 1, 0, 1):          # alternate: the second pair is the one reported
                lib.sidlsg_debug_set_attn_bwd_fused.raw(mode)
                g = torch.zeros_like(qkv)
                dq, dk, dv = (g.data_ptr() + 2 * C * i for i in range(3))

                def call():
                    getattr(lib, 'sidlsg_attn_bwd' + sfx)(q, k, v, o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq, dk, dv, delta.data_ptr(),
                                                          B, heads, N, N, D, 3 * C, 3 * C, 3 * C, C, N * 3 * C, N * 3 * C, N * 3 * C, N * C, s)
                res[mode] = (timeit(call), g)
            takes = lib.sidlsg_attn_bwd_fused_takes.raw(B, heads, N, N, D, 1)
            t0, t1 = res[0][0], res[1][0]
            g0, g1 = res[0][1].float(), res[1][1].float()
            d = [float((g1[..., i * C:(i + 1) * C] - g0[..., i * C:(i + 1) * C]).norm() / g0[..., i * C:(i + 1) * C].norm()) for i in range(3)]
            print(f"N{N} h{heads} d{D} B{B:<2d} {'ps   ' if ps else 'plain'}: two-kernel {t0:8.1f} us   fused(takes={takes}) {t1:8.1f} us   "
                  f"fused/two {t1 / t0:.3f}   rel-l2 fused vs two-kernel dq {d[0]:.2e} dk {d[1]:.2e} dv {d[2]:.2e}", flush=True)
            del qkv, do, o, g0, g1, res
    lib.sidlsg_debug_set_attn_bwd_fused.raw(old)


if __name__ == '__main__':
    main()
