"""fp8-frozen step: grouped e4m3 fake-score + teacher pass (SIDLSG_GROUPED_FROZEN=1) against the two-stream path (=0), alternating in one
session, one fresh process per run; plus one bf16 run for orientation and the pair pass timed next to the two single passes.

    python tools/ab/fp8_grouped_ab.py [--runs 3] [--arch sd21-base] [--out profiles/fp8_grouped_ab.txt]

Every child runs under its own time limit and the first failure ends the script (nothing more is started on the GPU).  The decision rule
for SiDStep.GROUP_E4M3_BY_DEFAULT is printed with the figures: group by default only if the grouped arm's mean beats the two-stream arm's by
more than the larger within-arm spread (max - min)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def passes(arch):
    """child: the e4m3 teacher pass, the e4m3 fake-score pass and the grouped pair pass on the CFG batch of the bench workload."""
    sys.path.insert(0, ROOT)
    import torch
    from sid_lsg_amd import ops
    from sid_lsg_amd.scheduler import DDPMScheduler
    from sid_lsg_amd.sd_util import hip_denoise, hip_prepare_denoise
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    dev = torch.device('cuda')
    b, lat, kappa = 8, 64, 1.5
    cfg = CONFIGS[arch]
    phi = HipUNet2DCondition(cfg).materialize(dev, seed=0, with_grad_buffers=False).requires_grad_(False)
    psi = HipUNet2DCondition(cfg).materialize(dev, seed=1, with_grad_buffers=False).requires_grad_(False)
    phi.enable_fp8_weights()
    psi.enable_fp8_weights(frozen_passes_only=True)
    sched = DDPMScheduler().to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    ctx = torch.randn(b, cfg.text_len, cfg.cross_attention_dim, device=dev, generator=g).to(torch.bfloat16)

    def timed(fn, n=10):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    with torch.no_grad():
        prep = hip_prepare_denoise(torch.randn(b, 4, lat, lat, device=dev, generator=g), torch.randn(b, 4, lat, lat, device=dev, generator=g),
                                   torch.randint(20, 980, (b,), device=dev, generator=g), ctx, ctx.clone(), sched, True)

        def single_psi():
            with psi.fp8_forward():
                hip_denoise(psi, prep, kappa, predict_x0=True)

        def pair():
            ef, er = psi.forward_pair(phi, prep.xin, prep.tt, prep.ctx)
            ops.cfg_x0(ef, prep.xt, prep.s0, prep.s1, kappa, True, torch.bfloat16)
            ops.cfg_x0(er, prep.xt, prep.s0, prep.s1, kappa, True, torch.bfloat16)
        t_phi = timed(lambda: hip_denoise(phi, prep, kappa, predict_x0=True))
        t_psi = timed(single_psi)
        t_pair = timed(pair)
    print(json.dumps(dict(teacher_ms=t_phi, fake_score_ms=t_psi, pair_ms=t_pair)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--arch', default='sd21-base')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fp8_grouped_ab.txt'))
    ap.add_argument('--limit', type=int, default=240, help='time limit of one child, seconds')
    args = ap.parse_args()
    lines = [f'# fp8-frozen step on one MI355X: SIDLSG_GROUPED_FROZEN=1 (grouped e4m3 fake-score + teacher pass) vs =0 (two streams: the behaviour before the',
             f'# grouped e4m3 launches existed), `bench.py --gpus 1 --arch {args.arch} --teacher-weights fp8-frozen`, {args.runs} runs per arm, alternating in one session,',
             '# one process per run (tools/ab/fp8_grouped_ab.py)']

    def child(cmd, env_extra):
        env = dict(os.environ, **env_extra)
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f'{cmd} failed with {r.returncode}: stopping')
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])

    def bench(mode, tw):
        out = child([sys.executable, 'bench.py', '--gpus', '1', '--arch', args.arch, '--teacher-weights', tw], {'SIDLSG_GROUPED_FROZEN': mode})
        line = (f'{tw:10s} GROUPED_FROZEN={mode}: {out["value"]:.2f} images/s  {out["ms_per_step"]:.2f} ms/step  grouped_frozen_pass={out["grouped_frozen_pass"]}  '
                f'loss_fake {out["loss_fake"]:.4f} loss_G {out["loss_G"]:.4f}')
        print(line, flush=True)
        lines.append(line)
        return out
    arms = {'0': [], '1': []}
    for _ in range(args.runs):
        for mode in ('0', '1'):
            out = bench(mode, 'fp8-frozen')
            assert out['grouped_frozen_pass'] == (mode == '1')
            arms[mode].append(out['value'])
    bench('auto', 'bf16')
    mean = {m: sum(v) / len(v) for m, v in arms.items()}
    spread = {m: max(v) - min(v) for m, v in arms.items()}
    gain = mean['1'] - mean['0']
    by_default = gain > max(spread.values())
    lines += [f'two-stream: mean {mean["0"]:.2f} images/s, spread (max - min) {spread["0"]:.2f};  grouped: mean {mean["1"]:.2f} images/s, spread {spread["1"]:.2f}',
              f'grouped - two-stream = {gain:+.2f} images/s ({100 * gain / mean["0"]:+.1f} %) against the larger within-arm spread {max(spread.values()):.2f}: '
              + ('beyond it -> SIDLSG_GROUPED_FROZEN=auto groups e4m3 pairs' if by_default else
                 'not beyond it -> SIDLSG_GROUPED_FROZEN=auto keeps the two-stream path for e4m3 pairs; =1 opts in')]
    p = child([sys.executable, os.path.abspath(__file__), 'passes', args.arch], {})
    lines.append(f'passes on the CFG batch of 16 samples (batch_gpu 8), e4m3 copies, no grad: teacher {p["teacher_ms"]:.2f} ms, fake score {p["fake_score_ms"]:.2f} ms, '
                 f'grouped pair pass {p["pair_ms"]:.2f} ms ({(p["teacher_ms"] + p["fake_score_ms"]) / p["pair_ms"]:.2f}x the two one after the other)')
    print('\n'.join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == 'passes':
        passes(sys.argv[2])
    else:
        main()
