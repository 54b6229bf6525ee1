"""The tiny40 SiD step of tests/test_gpu_deterministic.py in deterministic mode: 2 iterations x 2 accumulation rounds from fresh
networks.  run_step() is called in-process by the test; `python tests/det_step_worker.py OUT.pt {bf16|fp32}` runs it in a fresh
process (with whatever SIDLSG_* environment the test gives it) and saves the result."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_step(dtype=torch.bfloat16, dev='cuda'):
    from sid_lsg_amd import ops
    from sid_lsg_amd.optim import FusedAdamEMA
    from sid_lsg_amd.scheduler import DDPMScheduler
    from sid_lsg_amd.sid_step import SiDStep
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    dev = torch.device(dev)
    ops.ensure_workspace(dev)
    cfg, lat, b, lr = CONFIGS['tiny40'], 16, 2, 2e-5
    with ops.deterministic(True):
        phi = HipUNet2DCondition(cfg, compute_dtype=dtype).materialize(dev, seed=1).requires_grad_(False)
        psi = HipUNet2DCondition(cfg, compute_dtype=dtype).materialize(dev, seed=2)
        G = phi.clone_network()
        G_ema = phi.clone_network(with_grad_buffers=False)
        opt_f, opt_g = FusedAdamEMA(psi.parameters(), lr=lr), FusedAdamEMA(G.parameters(), lr=lr)
        step = SiDStep(G, psi, phi, G_ema, DDPMScheduler().to(dev), opt_f, opt_g, alpha=1.0, cfg_train_fake=1.5, cfg_eval_fake=1.5,
                       cfg_eval_real=4.5, batch_gpu_total=2 * b, init_timestep=625)
        gen = torch.Generator().manual_seed(3)
        losses = []
        for _ in range(2):
            inputs = {ph: [dict(z=torch.randn(b, 4, lat, lat, generator=gen).to(dev), noise=torch.randn(b, 4, lat, lat, generator=gen).to(dev),
                                t=torch.randint(20, 980, (b,), generator=gen).to(dev),
                                cond=torch.randn(b, cfg.text_len, cfg.cross_attention_dim, generator=gen).to(dev).to(dtype),
                                uncond=torch.randn(b, cfg.text_len, cfg.cross_attention_dim, generator=gen).to(dev).to(dtype)) for _ in range(2)]
                      for ph in ('A', 'B')}
            lf, lg = step.iteration(inputs, ema_beta=0.5)
            losses += [lf.detach().float().reshape(1), lg.detach().float().reshape(1)]
        torch.cuda.synchronize()
    out = dict(losses=torch.cat(losses), G=G.flat_params, psi=psi.flat_params, ema=G_ema.flat_params,
               G_sq=opt_g.exp_avg_sq, psi_sq=opt_f.exp_avg_sq)
    for name, opt in (('G_m', opt_g), ('psi_m', opt_f)):
        if opt.exp_avg is not None:
            out[name] = opt.exp_avg
    return {k: v.detach().cpu().clone() for k, v in out.items()}


if __name__ == '__main__':
    res = run_step(torch.float32 if sys.argv[2] == 'fp32' else torch.bfloat16)
    torch.save(res, sys.argv[1])
