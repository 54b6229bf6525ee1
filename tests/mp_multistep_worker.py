"""Child processes of tests/test_gpu_multistep.py (multi-step generator, N = 2).
    python tests/mp_multistep_worker.py rccl1             the step with the gradient exchange forced on RCCL at world 1
    torch.distributed.run ... mp_multistep_worker.py ddp2 <out>
                                                         INTEGRATION.md mode 2: G wrapped in DistributedDataParallel and handed to
                                                         the N-step sampler; 2 gloo ranks share cuda:0; each rank writes
                                                         <out>.rank<r>.npz"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def run_rccl1():
    import torch.distributed as tdist
    from sid_lsg_amd.distributed import FlatGradReducer
    from test_gpu_multistep import _assert_same_run, _step_run
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    tdist.init_process_group('nccl', rank=0, world_size=1)
    try:
        a, lr = _step_run(dev)
        e, _ = _step_run(dev, reducer=FlatGradReducer(min_world=1))
        e2, _ = _step_run(dev, reducer=FlatGradReducer(min_world=1), early=False)
        _assert_same_run(a, e, lr, 2, 2e-3)
        _assert_same_run(a, e2, lr, 2, 2e-3)
    finally:
        tdist.destroy_process_group()
    print('rccl1 ok', flush=True)


def run_ddp2(out):
    import torch.distributed as tdist
    from sid_lsg_amd.scheduler import DDPMScheduler
    from sid_lsg_amd.sd_util import hip_generate_steps
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    tdist.init_process_group('gloo')
    rank, world = tdist.get_rank(), tdist.get_world_size()
    cfg, b, lat, n = CONFIGS['tiny'], 2, 8, 2
    sched = DDPMScheduler().to(dev)
    G = HipUNet2DCondition(cfg).materialize(dev, seed=5).train().requires_grad_(True)
    ddp = torch.nn.parallel.DistributedDataParallel(G, device_ids=[dev], broadcast_buffers=False, find_unused_parameters=False)
    g = torch.Generator().manual_seed(200 + rank)                # the ranks see different inputs
    z = torch.randn(b, 4, lat, lat, generator=g).to(dev)
    eps_next = torch.randn(n - 1, b, 4, lat, lat, generator=g).to(dev)
    ctx = torch.randn(b, cfg.text_len, cfg.cross_attention_dim, generator=g).to(dev).to(torch.bfloat16)
    w = torch.randn(b, 4, lat, lat, generator=g).to(dev)
    init_t = torch.full((b,), 625, dtype=torch.long, device=dev)
    calls = [0]
    orig = tdist.all_reduce

    def counting_all_reduce(t, *a, **k):
        if t.data_ptr() == G.flat_grads.data_ptr():
            calls[0] += 1
        return orig(t, *a, **k)
    tdist.all_reduce = counting_all_reduce

    def backward():
        G.flat_grads.zero_()
        (hip_generate_steps(ddp, z, eps_next, ctx, init_t, sched) * w).sum().backward()
        torch.cuda.synchronize()
        return G.flat_grads.clone()
    with ddp.no_sync():
        local = backward()                      # no exchange under no_sync
    n_nosync = calls[0]
    calls[0] = 0
    synced = backward()                         # one exchange after the whole N-step backward
    n_sync = calls[0]
    tdist.all_reduce = orig
    mean = local.clone()
    tdist.all_reduce(mean)
    mean /= world
    err = float((synced - mean).abs().max() / mean.abs().max())
    local_vs_mean = float((local - mean).abs().max() / mean.abs().max())
    np.savez(f'{out}.rank{rank}.npz', n_nosync=n_nosync, n_sync=n_sync, err=err, local_vs_mean=local_vs_mean)
    tdist.destroy_process_group()


if __name__ == '__main__':
    if sys.argv[1] == 'rccl1':
        run_rccl1()
    elif sys.argv[1] == 'ddp2':
        run_ddp2(sys.argv[2])
    else:
        raise SystemExit(f'unknown mode {sys.argv[1]!r}')
