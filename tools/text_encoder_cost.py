#!/usr/bin/env python
"""Cost of the CLIP text encoder: text.HipCLIPTextModel (HIP kernels) against text.CLIPTextModel (PyTorch), the module it can replace.
    python tools/text_encoder_cost.py encode:sd15 | encode:sd21-base | bench
One part per process, so that each runs under a time limit of its own (`timeout 300 python tools/text_encoder_cost.py encode:sd15`).
encode:<arch>  the text configuration of <arch> (text.TEXT_CONFIGS), seeded weights, 77 hash-tokenizer ids per prompt, bf16 and fp32
               parameters, batches 1, 8 and 64 in one process: time per encode of both modules (device events around windows of
               back-to-back calls after warm-up, five windows per variant, the variants alternating; median and range), the largest
               difference of their outputs, and the kernel launches of one encode of each (torch profiler, in a pass of its own)
bench          one same-session A/B of the flagship benchmark: `python bench.py --gpus 1 --steps 20 --warmup 5` against the same
               command under SIDLSG_TEXT_ENCODER=hip, as child processes, alternating, two runs each; images/s of every run
Each line is printed and appended to profiles/text_encoder.txt."""
import copy
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'text_encoder.txt')
BATCHES = (1, 8, 64)


def say(line):
    print(line, flush=True)
    with open(OUT, 'a') as f:
        f.write(line + '\n')


def window_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / calls


def launches(fn):
    """Kernel launches of one call: the device-side kernel events of a torch profiler pass (not timed)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower() and
             'memset' not in e.name.lower()]
    if not names:
        raise RuntimeError('the profiler recorded no kernel: launches cannot be counted here')
    return len(names), sum('Cijk_' in n for n in names)


def encode(arch):
    from sid_lsg_amd.text import TEXT_CONFIGS, CLIPTextModel, HashTokenizer, HipCLIPTextModel
    dev = torch.device('cuda:0')
    say(f'--- text_encoder_cost.py encode:{arch}: {torch.cuda.get_device_name(0)}')
    torch.manual_seed(1)
    base = CLIPTextModel(**TEXT_CONFIGS[arch]).requires_grad_(False).eval()
    tok = HashTokenizer()
    for dtype, tag in ((torch.bfloat16, 'bf16'), (torch.float32, 'fp32')):
        te = copy.deepcopy(base).to(dtype).to(dev)
        hip = HipCLIPTextModel.from_torch(copy.deepcopy(te))
        ids = {b: tok([f'a photo of object number {i} on a table' for i in range(b)]).input_ids.to(dev) for b in BATCHES}
        variants = [(f'{name}, batch {b}', (lambda m=m, b=b: m(ids[b])[0])) for b in BATCHES for name, m in (('torch', te), ('hip', hip))]
        with torch.no_grad():
            for b in BATCHES:
                a, h = te(ids[b])[0].float(), hip(ids[b])[0].float()
                say(f'{arch} {tag} batch {b}: max |hip - torch| {float((a - h).abs().max()):.3e} (max |torch| {float(a.abs().max()):.3e})')
            for _, fn in variants:
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            samples = {name: [] for name, _ in variants}
            calls = 30
            for _ in range(5):
                for name, fn in variants:
                    samples[name].append(window_us(fn, calls))
            for name, v in samples.items():
                say(f'{arch} {tag}: {name}: {statistics.median(v):.1f} us per encode (median of 5 windows of {calls} calls, alternating; '
                    f'range {min(v):.1f} .. {max(v):.1f})')
            for name, m in (('torch', te), ('hip', hip)):
                n, blaslt = launches(lambda: m(ids[8])[0])
                say(f'{arch} {tag}: {name}: {n} kernel launches per encode (batch 8), {blaslt} of them Cijk_* (hipBLASLt)')
        del te, hip


def bench():
    say('--- text_encoder_cost.py bench: python bench.py --gpus 1 --steps 20 --warmup 5, default (torch text encoder) against '
        'SIDLSG_TEXT_ENCODER=hip, child processes, alternating')
    rates = {'torch': [], 'hip': []}
    for rnd in range(2):
        for kind in ('torch', 'hip'):
            env = dict(os.environ)
            env.pop('SIDLSG_TEXT_ENCODER', None)
            if kind == 'hip':
                env['SIDLSG_TEXT_ENCODER'] = 'hip'
            res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'], cwd=ROOT, env=env,
                                 capture_output=True, text=True, timeout=400)
            if res.returncode != 0:
                raise SystemExit(f'bench.py ({kind}) failed with code {res.returncode}:\n{res.stdout[-2000:]}{res.stderr[-2000:]}')
            line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith('{')][-1])
            rates[kind].append(line['value'])
            say(f'bench.py, round {rnd + 1}, text encoder {kind}: {line["value"]:.3f} images/s ({line["ms_per_step"]:.2f} ms per step, '
                f'loss_fake {line.get("loss_fake")}, loss_G {line.get("loss_G")})')
    say(f'bench.py: torch {statistics.mean(rates["torch"]):.3f} images/s, hip {statistics.mean(rates["hip"]):.3f} images/s (means of 2 runs)')


if __name__ == '__main__':
    part = sys.argv[1] if len(sys.argv) > 1 else ''
    if part.startswith('encode:') and part.split(':', 1)[1] in ('sd15', 'sd21-base'):
        encode(part.split(':', 1)[1])
    elif part == 'bench':
        bench()
    else:
        raise SystemExit(__doc__)
