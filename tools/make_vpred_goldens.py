"""Golden vectors of the v-prediction (SD 2.x 768-v) teacher path.  AUTHORING ONLY: needs the reference checkout.

    python tools/make_vpred_goldens.py [loops] [glue] [fullsize [<latent>]]      -> tests/golden/

  loop_v_<name>.npz          the UNMODIFIED reference training_loop (oracle.ref_harness) on the tiny seeded networks with the
                             scheduler swapped for a v-prediction restatement (VPredSchedulerRef); same schema as loop_*.npz.
                             batch_gpu = 1 throughout: the reference's `loss * snr / (snr + 1)` (sid_training_loop.py:440-441)
                             multiplies a [B,4,h,w] tensor by a [B] one, which broadcasts over the WIDTH axis and is only the
                             per-sample weight at B = 1 ("v-prediction").  Accumulation is exercised by
                             several rounds per iteration instead.
  glue_v_tiny.npz            the reference sid_sd_sampler / sid_sd_denoise under the v scheduler (kappa 1 and > 1, predict_x0
                             both ways); same schema as glue_tiny.npz.
  fullsize_sd21v_k2_<res>.npz  one full-size SD2.1 iteration of the CPU oracle pieces (oracle.fixtures seeded nets and inputs,
                             oracle.sid_ref sampler / denoise / generator loss / Adam / EMA) with the v scheduler and a per-sample
                             v fake-score loss (vpred_fake_loss_ref); schema of the existing fullsize_*.npz.

Nothing under oracle/ is modified: its modules are imported and the v pieces are restated here.
"""
import copy
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import fixtures, ref_harness, sid_ref  # noqa: E402
from oracle.make_goldens import PROMPTS  # noqa: E402
from oracle.scheduler_ref import DDPMSchedulerRef  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')


class VPredSchedulerRef(DDPMSchedulerRef):
    """DDPMSchedulerRef with prediction_type 'v_prediction': the published DDIM formulas the reference reaches through
    DDIMScheduler (sid_sd_util.py:66-68): step().pred_original_sample = sqrt(abar) x_t - sqrt(1 - abar) v, and
    get_velocity(x0, noise, t) = sqrt(abar) noise - sqrt(1 - abar) x0."""

    def __init__(self, **kw):
        super().__init__(prediction_type='v_prediction', **kw)

    def step(self, model_output, timestep, sample, return_dict=True):
        t = timestep if torch.is_tensor(timestep) else torch.tensor(timestep)
        ac = self.alphas_cumprod.to(device=sample.device, dtype=sample.dtype)[t.to(sample.device)]
        return SimpleNamespace(pred_original_sample=ac ** 0.5 * sample - (1 - ac) ** 0.5 * model_output)

    def get_velocity(self, sample, noise, timesteps):
        s0, s1 = self._coef(timesteps, sample)
        return s0 * noise - s1 * sample


def vpred_factory(cfg_name='tiny'):
    unet, vae, _, te, tok = fixtures.factory(cfg_name)
    return unet, vae, VPredSchedulerRef(), te, tok


def vpred_fake_loss_ref(o, images, noise, t, sched, loss_scaling, batch_gpu_total):
    """sid_training_loop.py:423-445 in v mode with the per-sample weight w_b = snr_b / (snr_b + 1) (snr from alphas_cumprod, as
    compute_snr): the reference's own expression at B = 1, its evident intent at any B."""
    target = sched.get_velocity(images, noise, t)
    nan_mask = torch.isnan(o).flatten(1).any(1) | torch.isnan(target).flatten(1).any(1)
    ac = sched.alphas_cumprod[t]
    snr = ac / (1 - ac)
    w = snr / (snr + 1)
    keep = ~nan_mask
    o, target, w = o[keep], target[keep], w[keep]
    loss = ((o - target) ** 2 * w.view(-1, 1, 1, 1)).sum() * (loss_scaling / batch_gpu_total)
    return loss, len(o)


def vpred_iteration_ref(nets, opt_states, sched, inputs, hp):
    """oracle.sid_ref.sid_iteration_ref with the v fake-score loss (phase A); phase B and the updates are its own pieces."""
    G, psi, phi = nets['G'], nets['fake_score'], nets['true_score']
    out = {}
    psi.requires_grad_(True)
    for r in inputs['A']:
        init_t = torch.full((len(r['z']),), hp['init_t'], dtype=torch.long)
        with torch.no_grad():
            images = sid_ref.sampler_ref(G, r['z'], r['cond'], init_t, sched)
        o = sid_ref.denoise_ref(psi, images, r['noise'], r['cond'], r['uncond'], r['t'], sched, predict_x0=False,
                                guidance_scale=hp['kappa1'])
        loss, n = vpred_fake_loss_ref(o, images, r['noise'], r['t'], sched, hp['ls'], hp['batch_gpu_total'])
        if n > 0:
            loss.backward()
    out['loss_fake'] = float(loss.detach())
    psi.requires_grad_(False)
    for p, st in zip(psi.parameters(), opt_states['fake_score']):
        if p.grad is not None:
            with torch.no_grad():
                sid_ref.adam_step_ref(p, p.grad, st, hp['lr'], hp['betas'], hp['eps'])
    G.requires_grad_(True)
    for r in inputs['B']:
        init_t = torch.full((len(r['z']),), hp['init_t'], dtype=torch.long)
        images = sid_ref.sampler_ref(G, r['z'], r['cond'], init_t, sched)
        y_fake = sid_ref.denoise_ref(psi, images, r['noise'], r['cond'], r['uncond'], r['t'], sched, guidance_scale=hp['kappa2'])
        y_real = sid_ref.denoise_ref(phi, images, r['noise'], r['cond'], r['uncond'], r['t'], sched, guidance_scale=hp['kappa4'])
        loss, n = sid_ref.generator_loss_ref(images, y_real, y_fake, hp['alpha'], hp['lsg'], hp['batch_gpu_total'])
        if n > 0:
            loss.backward()
    out['loss_G'] = float(loss.detach())
    G.requires_grad_(False)
    for p, st in zip(G.parameters(), opt_states['G']):
        if p.grad is not None:
            with torch.no_grad():
                sid_ref.adam_step_ref(p, p.grad, st, hp['glr'], hp['betas'], hp['eps'])
    beta = sid_ref.ema_beta_ref(hp['batch_size'], hp['cur_nimg'], hp['ema_halflife_kimg'], hp.get('ema_rampup_ratio', 0.05))
    with torch.no_grad():
        for pe, p in zip(nets['G_ema'].parameters(), G.parameters()):
            sid_ref.ema_update_ref(pe, p, beta)
    return out


# ---- loop goldens ---------------------------------------------------------------------------------------------------------
LOOPS = {
    # kappa 1.5 everywhere, 2 accumulation rounds of one sample, alpha 1
    'k15_a1': dict(iterations=4, batch_size=2, batch_gpu=1, seed=3, alpha=1.0, kappa=(1.5, 1.5, 1.5), lr=1e-4, glr=1e-4, resolution=128),
    # no guidance (single-branch path, no prompt dropout), alpha 1.2 general branch, 4 accumulation rounds
    'k1_a12': dict(iterations=3, batch_size=4, batch_gpu=1, seed=5, alpha=1.2, kappa=(1.0, 1.0, 1.0), lr=1e-5, glr=1e-5, resolution=128),
}


def gen_loops():
    for name, kw in LOOPS.items():
        with tempfile.TemporaryDirectory() as tmp:
            pdir = os.path.join(tmp, 'prompts')
            os.makedirs(pdir)
            with open(os.path.join(pdir, 'aesthetics_6_plus.txt'), 'wt') as f:
                f.write('\n'.join(PROMPTS) + '\n')
            run_dir = os.path.join(tmp, 'run')
            os.makedirs(run_dir)
            with ref_harness.cpu_process_group():
                res = ref_harness.run_reference_training_loop(lambda: vpred_factory('tiny'), pdir, run_dir, **kw)
        out = dict(cfg='tiny', prediction_type='v_prediction', prompts=np.array(PROMPTS),
                   loss_names=np.array([n for n, _ in res['losses']]),
                   loss_values=np.array([v for _, v in res['losses']], dtype=np.float64),
                   weight_checksum=np.array(fixtures.checksum(fixtures.make_unet('tiny'))),
                   fake_score_checksum=np.array(fixtures.checksum(res['fake_score_params'])),
                   G_checksum=np.array(fixtures.checksum(res['G_params'])),
                   G_conv_in_w=res['G_params'][0].numpy(), fake_conv_in_w=res['fake_score_params'][0].numpy(),
                   G_last_b=res['G_params'][-1].numpy(), fake_last_b=res['fake_score_params'][-1].numpy())
        for k, v in kw.items():
            out['kw_' + k] = np.array(v)
        np.savez_compressed(os.path.join(OUT, f'loop_v_{name}.npz'), **out)
        print('loop_v', name, [f'{v:.6g}' for v in out['loss_values']], flush=True)


# ---- glue golden ----------------------------------------------------------------------------------------------------------
def gen_glue():
    ref = ref_harness.import_reference()
    cfg_name, lat = 'tiny', 8
    unet, _, sched, te, tok = vpred_factory(cfg_name)
    unet2 = fixtures.make_unet(cfg_name, seed=99)
    unet.eval().requires_grad_(False)
    unet2.eval().requires_grad_(False)
    out = dict(cfg=cfg_name, prediction_type='v_prediction', weight_checksum=np.array(fixtures.checksum(unet)),
               weight_checksum2=np.array(fixtures.checksum(unet2)))
    g = torch.Generator().manual_seed(17)
    case = 0
    for b in (1, 2):
        prompts = PROMPTS[case:case + b]
        z = torch.randn(b, 4, lat, lat, generator=g)
        noise = torch.randn(b, 4, lat, lat, generator=g)
        t = torch.randint(20, 980, (b,), generator=g)
        init_t = torch.full((b,), 625, dtype=torch.long)
        xhat = ref.sd_util.sid_sd_sampler(unet=unet, latents=z, contexts=prompts, init_timesteps=init_t, noise_scheduler=sched,
                                          text_encoder=te, tokenizer=tok, resolution=lat * 8, dtype=torch.float32,
                                          return_images=False, vae=None, num_steps=1)
        out[f'b{b}_z'], out[f'b{b}_noise'], out[f'b{b}_t'] = z.numpy(), noise.numpy(), t.numpy()
        out[f'b{b}_prompts'] = np.array(prompts)
        out[f'b{b}_xhat'] = xhat.numpy()
        for kappa in (1.0, 2.0):
            for px0 in (True, False):
                y = ref.sd_util.sid_sd_denoise(unet=unet2, images=xhat, noise=noise, contexts=prompts, timesteps=t,
                                               noise_scheduler=sched, text_encoder=te, tokenizer=tok, resolution=lat * 8,
                                               dtype=torch.float32, predict_x0=px0, guidance_scale=kappa)
                out[f'b{b}_k{kappa}_x0{int(px0)}'] = y.detach().numpy()
        case += b
    np.savez_compressed(os.path.join(OUT, 'glue_v_tiny.npz'), **out)
    print('glue_v_tiny done', flush=True)


# ---- stored full-size iteration -------------------------------------------------------------------------------------------
def fullsize_case(lat):
    return ('sd21-base', lat, 1, 2.0)


def gen_fullsize(lat=96):
    cfg_name, lat, b, kappa = fullsize_case(lat)
    lr = fixtures.FULLSIZE_LR
    t0 = time.time()
    phi_r = fixtures.make_unet_cached(cfg_name).eval().requires_grad_(False)
    psi_r = fixtures.make_unet_cached(cfg_name, seed=77).requires_grad_(False)
    G_r = copy.deepcopy(phi_r)
    Gema_r = copy.deepcopy(G_r)
    init = {'fake_score': [p.detach().clone() for p in psi_r.parameters()], 'G': [p.detach().clone() for p in G_r.parameters()]}
    cks = np.array(fixtures.checksum(phi_r) + fixtures.checksum(psi_r))
    nets_r = dict(true_score=phi_r, fake_score=psi_r, G=G_r, G_ema=Gema_r)
    st = dict(fake_score=[{} for _ in psi_r.parameters()], G=[{} for _ in G_r.parameters()])
    hp = fixtures.iteration_hp(b, 1, lr, kappa, 1.0)
    hp['cur_nimg'] = 0
    inputs = fixtures.iteration_inputs(cfg_name, lat, b, 1, torch.Generator().manual_seed(fixtures.FULLSIZE_SEED))
    out_r = vpred_iteration_ref(nets_r, st, VPredSchedulerRef(), inputs, hp)
    rec = dict(loss_fake=np.float64(out_r['loss_fake']), loss_G=np.float64(out_r['loss_G']), weight_checksum=cks,
               case=np.array([cfg_name, str(lat), str(b), str(kappa), str(lr)]), prediction_type='v_prediction')
    ema = dict(Gema_r.named_parameters())
    for n in fixtures.FULLSIZE_EMA_NAMES:
        rec['ema/' + n] = ema[n].detach().numpy().copy()
    for name, net in (('fake_score', psi_r), ('G', G_r)):
        sign, big = [], []
        for p, p0 in zip(net.parameters(), init[name]):
            idx = fixtures.sample_index(p.numel())
            d = (p.detach().flatten()[idx] - p0.flatten()[idx])
            sign.append((d > 0).numpy())
            big.append((d.abs() > 0.5 * lr).numpy())
        sign, big = np.concatenate(sign), np.concatenate(big)
        rec[name + '/n'] = np.int64(sign.size)
        rec[name + '/sign'] = np.packbits(sign)
        rec[name + '/big'] = np.packbits(big)
    path = os.path.join(OUT, f'fullsize_sd21v_k2_{lat * 8}.npz')
    np.savez_compressed(path, **rec)
    print(f'fullsize v {lat}x{lat}: loss_fake {out_r["loss_fake"]:.6f} loss_G {out_r["loss_G"]:.6f} -> {path} '
          f'({os.path.getsize(path) / 1e6:.2f} MB, {time.time() - t0:.0f} s)', flush=True)


if __name__ == '__main__':
    torch.set_num_threads(min(48, os.cpu_count() or 8))
    which = sys.argv[1:] or ['loops', 'glue', 'fullsize']
    if 'loops' in which:
        gen_loops()
    if 'glue' in which:
        gen_glue()
    if 'fullsize' in which:
        i = which.index('fullsize')
        gen_fullsize(int(which[i + 1]) if len(which) > i + 1 and which[i + 1].isdigit() else 96)
