"""Golden vectors of multi-step generator training (--num_steps N > 1).  AUTHORING ONLY: needs the reference checkout.

    python tools/make_multistep_goldens.py [loops] [glue]      -> tests/golden/

  loop_ns<N>_<name>.npz      the UNMODIFIED reference training_loop (oracle.ref_harness) on the tiny seeded networks with
  loop_v_ns<N>_<name>.npz    num_steps = N (extra=dict(num_steps=N)); same schema as loop_*.npz, plus the draws the loop made in
                             its FIRST iteration, captured by wrapping the loop module's sid_sd_sampler / sid_sd_denoise:
                             draw_<A|B>_z [R,B,4,h,w], draw_<A|B>_eps [R,N-1,B,4,h,w] (what torch.randn_like returned inside the
                             sampler), draw_<A|B>_noise [R,B,4,h,w], draw_<A|B>_t [R,B] for the R accumulation rounds of each phase.
                             The v variant swaps the scheduler for tools/make_vpred_goldens.VPredSchedulerRef.
  glue_ns_tiny.npz           the reference sid_sd_sampler(train_sampler=True, num_steps in {2, 4}) on the tiny oracle UNet, epsilon
                             and v: <p>_ns<N>_z, _eps (the eps_i it drew), _xhat, and the fp32 gradient of <x_hat, w> (w seeded,
                             stored as _w) on the parameters named in GRAD_NAMES (_grad/<name>).

The reference loop runs at N > 1 under the harness's world-1 DDP as written.  Nothing under oracle/ is modified.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from oracle import fixtures, ref_harness  # noqa: E402
from oracle.make_goldens import PROMPTS  # noqa: E402
from make_vpred_goldens import vpred_factory  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
GRAD_NAMES = ('conv_in.weight', 'conv_out.bias', 'time_embedding.linear_1.weight', 'mid_block.attentions.0.proj_in.weight')

# name -> (num_steps, prediction, loop kwargs); the kwargs are those of the one-step goldens of the same name
LOOPS = {
    'ns2_k15_a1': (2, 'epsilon', dict(iterations=4, batch_size=2, batch_gpu=1, seed=3, alpha=1.0, kappa=(1.5, 1.5, 1.5), lr=1e-4,
                                      glr=1e-4, resolution=128)),
    'ns4_k1_a12': (4, 'epsilon', dict(iterations=3, batch_size=4, batch_gpu=1, seed=5, alpha=1.2, kappa=(1.0, 1.0, 1.0), lr=1e-5,
                                      glr=1e-5, resolution=128)),
    'v_ns2_k15_a1': (2, 'v_prediction', dict(iterations=4, batch_size=2, batch_gpu=1, seed=3, alpha=1.0, kappa=(1.5, 1.5, 1.5),
                                             lr=1e-4, glr=1e-4, resolution=128)),
}


class _DrawRecorder:
    """Wraps the loop module's sid_sd_sampler / sid_sd_denoise: the training-sampler calls (train_sampler=True, no images) record z
    and every torch.randn_like result; the denoise calls record noise and t.  Only until `limit` sampler calls are recorded."""

    def __init__(self, loop_mod, limit):
        self.mod, self.limit = loop_mod, limit
        self.samples, self.denoises, self.calls = [], [], 0

    def __enter__(self):
        self.saved = (self.mod.sid_sd_sampler, self.mod.sid_sd_denoise)
        samp, den = self.saved

        def sampler(*a, **k):
            if not k.get('train_sampler', True) or k.get('return_images', False):
                return samp(*a, **k)
            self.calls += 1
            if self.calls > self.limit:
                return samp(*a, **k)
            drawn, orig = [], torch.randn_like

            def randn_like(*aa, **kk):
                x = orig(*aa, **kk)
                drawn.append(x.detach().clone())
                return x
            torch.randn_like = randn_like
            try:
                out = samp(*a, **k)
            finally:
                torch.randn_like = orig
            self.samples.append(dict(z=k['latents'].detach().clone(), eps=drawn))
            return out

        def denoise(*a, **k):
            if self.calls <= self.limit:
                self.denoises.append(dict(noise=k['noise'].detach().clone(), t=k['timesteps'].detach().clone(), n=self.calls))
            return den(*a, **k)
        self.mod.sid_sd_sampler, self.mod.sid_sd_denoise = sampler, denoise
        return self

    def __exit__(self, *exc):
        self.mod.sid_sd_sampler, self.mod.sid_sd_denoise = self.saved
        return False


def gen_loops():
    ref = ref_harness.import_reference()
    for name, (n, pt, kw) in LOOPS.items():
        rounds = kw['batch_size'] // kw['batch_gpu']
        factory = (lambda: vpred_factory('tiny')) if pt == 'v_prediction' else (lambda: fixtures.factory('tiny'))
        with tempfile.TemporaryDirectory() as tmp:
            pdir = os.path.join(tmp, 'prompts')
            os.makedirs(pdir)
            with open(os.path.join(pdir, 'aesthetics_6_plus.txt'), 'wt') as f:
                f.write('\n'.join(PROMPTS) + '\n')
            run_dir = os.path.join(tmp, 'run')
            os.makedirs(run_dir)
            with ref_harness.cpu_process_group(), _DrawRecorder(ref.loop, 2 * rounds) as rec:
                res = ref_harness.run_reference_training_loop(factory, pdir, run_dir, extra=dict(num_steps=n), **kw)
        out = dict(cfg='tiny', prediction_type=pt, num_steps=np.int64(n), prompts=np.array(PROMPTS),
                   loss_names=np.array([m for m, _ in res['losses']]),
                   loss_values=np.array([v for _, v in res['losses']], dtype=np.float64),
                   weight_checksum=np.array(fixtures.checksum(fixtures.make_unet('tiny'))),
                   fake_score_checksum=np.array(fixtures.checksum(res['fake_score_params'])),
                   G_checksum=np.array(fixtures.checksum(res['G_params'])),
                   G_conv_in_w=res['G_params'][0].numpy(), fake_conv_in_w=res['fake_score_params'][0].numpy(),
                   G_last_b=res['G_params'][-1].numpy(), fake_last_b=res['fake_score_params'][-1].numpy())
        for k, v in kw.items():
            out['kw_' + k] = np.array(v)
        # first iteration: phase A = sampler calls 0 .. R-1 (one denoise each), phase B = R .. 2R-1 (fake + real denoise, same inputs)
        assert len(rec.samples) == 2 * rounds, len(rec.samples)
        for ph, calls in (('A', range(rounds)), ('B', range(rounds, 2 * rounds))):
            zs, eps, noises, ts = [], [], [], []
            for c in calls:
                s = rec.samples[c]
                assert len(s['eps']) == n - 1, (name, c, len(s['eps']))
                d = [x for x in rec.denoises if x['n'] == c + 1]
                assert len(d) == (1 if ph == 'A' else 2), (name, c, len(d))
                zs.append(s['z'].numpy())
                eps.append(np.stack([e.numpy() for e in s['eps']]))
                noises.append(d[0]['noise'].numpy())
                ts.append(d[0]['t'].numpy())
            out[f'draw_{ph}_z'], out[f'draw_{ph}_eps'] = np.stack(zs), np.stack(eps)
            out[f'draw_{ph}_noise'], out[f'draw_{ph}_t'] = np.stack(noises), np.stack(ts)
        path = os.path.join(OUT, f'loop_{name}.npz')
        np.savez_compressed(path, **out)
        print('loop', name, [f'{v:.6g}' for v in out['loss_values']], f'{os.path.getsize(path) / 1e3:.0f} kB', flush=True)


def gen_glue():
    ref = ref_harness.import_reference()
    lat, b = 8, 2
    out = dict(cfg='tiny', grad_names=np.array(GRAD_NAMES), weight_checksum=np.array(fixtures.checksum(fixtures.make_unet('tiny'))))
    g = torch.Generator().manual_seed(29)
    prompts = PROMPTS[:b]
    out['prompts'] = np.array(prompts)
    init_t = torch.full((b,), 625, dtype=torch.long)
    for p, fac in (('eps', lambda: fixtures.factory('tiny')), ('v', lambda: vpred_factory('tiny'))):
        unet, _, sched, te, tok = fac()
        unet.train().requires_grad_(True)
        params = dict(unet.named_parameters())
        for n in (2, 4):
            z = torch.randn(b, 4, lat, lat, generator=g)
            w = torch.randn(b, 4, lat, lat, generator=g)
            torch.manual_seed(1000 + n)
            drawn, orig = [], torch.randn_like

            def randn_like(*aa, **kk):
                x = orig(*aa, **kk)
                drawn.append(x.detach().clone())
                return x
            for q in unet.parameters():
                q.grad = None
            torch.randn_like = randn_like
            try:
                xhat = ref.sd_util.sid_sd_sampler(unet=unet, latents=z, contexts=prompts, init_timesteps=init_t, noise_scheduler=sched,
                                                  text_encoder=te, tokenizer=tok, resolution=lat * 8, dtype=torch.float32,
                                                  return_images=False, vae=None, num_steps=n, train_sampler=True)
            finally:
                torch.randn_like = orig
            (xhat * w).sum().backward()
            k = f'{p}_ns{n}'
            out[k + '_z'], out[k + '_w'], out[k + '_xhat'] = z.numpy(), w.numpy(), xhat.detach().numpy()
            out[k + '_eps'] = np.stack([e.numpy() for e in drawn])
            for name in GRAD_NAMES:
                out[f'{k}_grad/{name}'] = params[name].grad.detach().numpy().copy()
            print('glue', k, 'eps drawn', len(drawn), 'xhat max', float(xhat.abs().max()), flush=True)
    path = os.path.join(OUT, 'glue_ns_tiny.npz')
    np.savez_compressed(path, **out)
    print('glue_ns_tiny', f'{os.path.getsize(path) / 1e3:.0f} kB', flush=True)


if __name__ == '__main__':
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    which = sys.argv[1:] or ['loops', 'glue']
    if 'glue' in which:
        gen_glue()
    if 'loops' in which:
        gen_loops()
