"""DDPM scheduler with the four members the reference touches (training/sid_sd_util.py:182-185,
191-195, 242-244, 262, 270; training/sid_training_loop.py:424,438): add_noise, scale_model_input,
step(...).pred_original_sample, config.prediction_type.  SD `scheduler_config.json` values:
scaled_linear betas 0.00085..0.012, 1000 steps, epsilon prediction, no sample clipping.

prediction_type 'v_prediction' (SD 2.x 768-v teachers): the reference swaps in DDIMScheduler for these
(sid_sd_util.py:66-68); its pred_original_sample is the same as DDPM's, sqrt(abar) x_t - sqrt(1-abar) v, so
one class serves both.  `from_config` takes a diffusers `scheduler_config.json` dict and refuses what it would
not reproduce exactly.

`coefficients(t)` returns the per-sample (sqrt(abar_t), sqrt(1-abar_t)) pair that the fused HIP glue
kernels (sidlsg_noisy_input / sidlsg_cfg_x0) consume, with no host synchronisation (the reference's
per-sample `scheduler.step` loop, sid_sd_util.py:270, costs 2*b host syncs per call).
"""
from types import SimpleNamespace

import torch


PREDICTION_TYPES = ('epsilon', 'v_prediction')


def prediction_mode(prediction_type):
    """The `mode` of sidlsg_cfg_x0 that turns a network output of this parameterisation into x0 (1 epsilon, 2 v)."""
    if prediction_type not in PREDICTION_TYPES:
        raise ValueError(f'prediction_type {prediction_type!r}: expected one of {PREDICTION_TYPES}')
    return 1 if prediction_type == 'epsilon' else 2


# what SD 1.x / 2.x `scheduler/scheduler_config.json` files say; used for seeded `random:<arch>` networks, which have no such file
SD_SAMPLING_CONFIG = dict(steps_offset=1, set_alpha_to_one=False, timestep_spacing='leading')


def ddim_schedule(scheduler, config_dict, num_inference_steps):
    """The timesteps and coefficients of an N-step deterministic DDIM sampler, by the index arithmetic of diffusers'
    DDIMScheduler.set_timesteps / step with timestep_spacing 'leading':
        ratio = T // N;  t_i = (N-1-i)*ratio + steps_offset;  prev_i = t_i - ratio;
        abar_prev = alphas_cumprod[prev_i] when prev_i >= 0, else the final value: 1 if set_alpha_to_one else alphas_cumprod[0].
    `config_dict`: the model's scheduler_config.json (keys steps_offset, default 0; set_alpha_to_one, default true;
    timestep_spacing, default 'leading'); None = diffusers' defaults.
    -> (timesteps LongTensor[N], s0, s1, s0p, s1p FloatTensor[N]) on the scheduler's device: sqrt(abar) and sqrt(1-abar) at t_i and
    at prev_i, fp32, from the scheduler's own fp32 alphas_cumprod.  Raises ValueError naming the key it refuses."""
    c = dict(config_dict or {})
    spacing = c.get('timestep_spacing', 'leading')
    if spacing != 'leading':
        raise ValueError(f"timestep_spacing={spacing!r}: only 'leading' is reproduced")
    T = int(scheduler.config.num_train_timesteps)
    N = int(num_inference_steps)
    if N < 1:
        raise ValueError(f'num_inference_steps={N}: expected at least 1')
    if N > T:
        raise ValueError(f'num_inference_steps={N}: more than num_train_timesteps={T}')
    offset = int(c.get('steps_offset', 0))
    ratio = T // N
    t0 = (N - 1) * ratio + offset
    if t0 >= T or offset < 0:
        raise ValueError(f'steps_offset={offset}: the first timestep {t0} is outside [0, {T}) for num_inference_steps={N}')
    abar = scheduler.alphas_cumprod
    t = torch.arange(N - 1, -1, -1, dtype=torch.long, device=abar.device) * ratio + offset
    prev = t - ratio
    final = torch.ones((), dtype=abar.dtype, device=abar.device) if c.get('set_alpha_to_one', True) else abar[0]
    abar_prev = torch.where(prev >= 0, abar[prev.clamp(min=0)], final)
    abar_t = abar[t]
    return t, abar_t ** 0.5, (1 - abar_t) ** 0.5, abar_prev ** 0.5, (1 - abar_prev) ** 0.5


SOLVERS = ('ddim', 'dpmpp2m')
SPACINGS = ('leading', 'trailing', 'linspace')


def solver_tables(scheduler, config_dict, num_inference_steps, solver='dpmpp2m', spacing=None, eta=0.0, start=0):
    """The timesteps and update coefficients of an N-step teacher sampler for sidlsg_solver_step.  One step from s (now) to t
    (target) is  x_t = c_x*x_s + c_cur*x0_s + c_prev*x0_r + c_n*xi  with x0_s the x0 prediction at s, x0_r that of the step before
    and xi fresh N(0, 1) noise.  With abar the scheduler's alphas_cumprod, alpha = sqrt(abar), sigma = sqrt(1 - abar),
    lambda = (ln abar - ln(1 - abar)) / 2, T = num_train_timesteps and numpy's half-to-even `round`:

      solver 'ddim' (Song et al. 2021, any eta >= 0), spacing 'leading' (ddim_schedule's arithmetic) or 'trailing'
      (t_i = round(T - i*T/N) - 1); the target of step i is t_i - T//N, below 0 the final abar (1 if set_alpha_to_one else abar[0]):
        sigma_eta = eta*sqrt((1 - abar_t)/(1 - abar_s))*sqrt(1 - abar_s/abar_t)   (0 on a step onto abar = 1)
        c_x = sqrt(sigma_t^2 - sigma_eta^2)/sigma_s;  c_cur = alpha_t - c_x*alpha_s;  c_prev = 0;  c_n = sigma_eta
      solver 'dpmpp2m' (DPM-Solver++ 2M, Lu et al. 2022: data prediction, order 2, midpoint, final sigma = 0), spacing 'leading'
      (t_i = (N - i)*(T//(N + 1)) + steps_offset), 'trailing' (as above) or 'linspace' (round(linspace(0, T - 1, N + 1)) reversed,
      last entry dropped); the target of step i is t_{i+1}, that of the last step the clean state abar = 1:
        h = lambda_t - lambda_s;  A = alpha_t*(1 - exp(-h));  c_x = sigma_t/sigma_s;  c_n = 0
        step 0:          c_cur = A;  c_prev = 0
        steps 1 .. N-2:  r0 = (lambda_s - lambda_r)/h with r the point before s;  c_cur = A*(1 + 0.5/r0);  c_prev = -A*0.5/r0
      any step onto abar = 1 (dpmpp2m's last one): the row (0, 1, 0, 0) exactly -- x_t is the x0 prediction, no lambda = inf is formed.

    These rules restate diffusers 0.27.2's DDIMScheduler and DPMSolverMultistepScheduler; agreement with the package is not pinned
    by a test.  `start` = k (image-to-image: the chain is entered at step k, 0 <= k < N, sd_util.teacher_start_index): 'dpmpp2m' has no
    x0 history at its first executed step, so row k is the first-order row (sigma_t/sigma_s, A, 0, 0) that step 0 has; every other row,
    the timesteps and alpha / sigma do not depend on it, and 'ddim' has no history at all.  The tables keep N rows, the loop indexes
    them from k.  `config_dict` as ddim_schedule (steps_offset, set_alpha_to_one, timestep_spacing); `spacing` None takes its
    timestep_spacing.  All arithmetic is fp64 from the scheduler's own fp32 alphas_cumprod.
    -> numpy (timesteps int64[N], alpha f64[N], sigma f64[N] at t_i, coef f64[N, 4] = (c_x, c_cur, c_prev, c_n)); solver_schedule
    rounds them to fp32 once.  Raises ValueError naming the argument it refuses."""
    import numpy as np
    c = dict(config_dict or {})
    if solver not in SOLVERS:
        raise ValueError(f'solver={solver!r}: expected one of {SOLVERS}')
    if spacing is None:
        spacing = c.get('timestep_spacing', 'leading')
    if spacing not in SPACINGS:
        raise ValueError(f'spacing={spacing!r}: expected one of {SPACINGS}')
    if solver == 'ddim' and spacing == 'linspace':
        raise ValueError("spacing='linspace': not reproduced for solver='ddim' (use 'leading' or 'trailing')")
    eta = float(eta)
    if not eta >= 0 or eta == float('inf'):
        raise ValueError(f'eta={eta}: expected a finite value >= 0')
    if solver == 'dpmpp2m' and eta != 0:
        raise ValueError(f"eta={eta}: solver='dpmpp2m' is deterministic (eta applies to solver='ddim')")
    T = int(scheduler.config.num_train_timesteps)
    N = int(num_inference_steps)
    if N < 1:
        raise ValueError(f'num_inference_steps={N}: expected at least 1')
    if N > T:
        raise ValueError(f'num_inference_steps={N}: more than num_train_timesteps={T}')
    start = int(start)
    if not 0 <= start < N:
        raise ValueError(f'start={start}: expected a step in [0, {N})')
    offset = int(c.get('steps_offset', 0))
    i = np.arange(N, dtype=np.int64)
    if spacing == 'trailing':
        t = np.round(T - i.astype(np.float64) * (T / N)).astype(np.int64) - 1
    elif spacing == 'linspace':
        t = np.round(np.linspace(0, T - 1, N + 1))[::-1][:-1].astype(np.int64)
    elif solver == 'ddim':
        t = (N - 1 - i) * (T // N) + offset
    else:
        t = (N - i) * (T // (N + 1)) + offset
    if spacing == 'leading' and (offset < 0 or t[0] >= T):
        raise ValueError(f'steps_offset={offset}: the first timestep {int(t[0])} is outside [0, {T}) for num_inference_steps={N}')
    if t.min() < 0 or t.max() >= T or np.any(np.diff(t) >= 0):
        raise ValueError(f'num_inference_steps={N}: the timesteps of solver={solver!r}, spacing={spacing!r} are not strictly decreasing '
                         f'inside [0, {T})')
    abar_dev = scheduler.alphas_cumprod
    abar = abar_dev.detach().cpu().to(torch.float64).numpy()
    a_s = abar[t]
    if solver == 'ddim':
        prev = t - T // N
        final = 1.0 if c.get('set_alpha_to_one', True) else abar[0]
        a_t = np.where(prev >= 0, abar[np.maximum(prev, 0)], final)
    else:
        a_t = np.append(abar[t[1:]], 1.0)
    coef = np.zeros((N, 4), dtype=np.float64)
    lam = lambda a: 0.5 * (np.log(a) - np.log1p(-a))  # noqa: E731
    for k in range(N):
        if a_t[k] == 1.0:
            coef[k] = (0.0, 1.0, 0.0, 0.0)
            continue
        al_s, sg_s, al_t, sg_t = np.sqrt(a_s[k]), np.sqrt(1 - a_s[k]), np.sqrt(a_t[k]), np.sqrt(1 - a_t[k])
        if solver == 'ddim':
            sg_eta = eta * np.sqrt((1 - a_t[k]) / (1 - a_s[k])) * np.sqrt(max(1 - a_s[k] / a_t[k], 0.0))
            if sg_eta > sg_t:
                raise ValueError(f'eta={eta}: sigma_eta exceeds sigma_t at step {k} (t = {int(t[k])})')
            cx = np.sqrt(sg_t ** 2 - sg_eta ** 2) / sg_s
            coef[k] = (cx, al_t - cx * al_s, 0.0, sg_eta)
        else:
            h = lam(a_t[k]) - lam(a_s[k])
            A = -al_t * np.expm1(-h)
            if k == start or k == 0:
                coef[k] = (sg_t / sg_s, A, 0.0, 0.0)
            else:
                r0 = (lam(a_s[k]) - lam(a_s[k - 1])) / h
                coef[k] = (sg_t / sg_s, A * (1 + 0.5 / r0), -A * 0.5 / r0, 0.0)
    return t.copy(), np.sqrt(a_s), np.sqrt(1 - a_s), coef


def solver_schedule(scheduler, config_dict, num_inference_steps, solver='dpmpp2m', spacing=None, eta=0.0, start=0):
    """solver_tables rounded to fp32 once, as the tensors sidlsg_solver_step takes:
    -> (timesteps Long[N], s0 f32[N], s1 f32[N], coef f32[N, 4]) on the scheduler's device, s0 / s1 being alpha / sigma at t_i."""
    t, al, sg, coef = solver_tables(scheduler, config_dict, num_inference_steps, solver=solver, spacing=spacing, eta=eta, start=start)
    dev = scheduler.alphas_cumprod.device
    f32 = lambda v: torch.from_numpy(v).to(torch.float32).to(dev)  # noqa: E731
    return torch.from_numpy(t).to(dev), f32(al), f32(sg), f32(coef)


class DDPMScheduler:
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, prediction_type='epsilon',
                 beta_schedule='scaled_linear'):
        prediction_mode(prediction_type)
        if beta_schedule == 'scaled_linear':
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == 'linear':
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise ValueError(f'beta_schedule {beta_schedule!r}: expected scaled_linear or linear')
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self._s0 = self.alphas_cumprod ** 0.5
        self._s1 = (1 - self.alphas_cumprod) ** 0.5
        snr = self.alphas_cumprod / (1 - self.alphas_cumprod)        # as diffusers' compute_snr
        self._w = snr / (snr + 1)
        self.config = SimpleNamespace(prediction_type=prediction_type, num_train_timesteps=num_train_timesteps,
                                      beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                                      clip_sample=False)

    @classmethod
    def from_config(cls, config):
        """A diffusers `scheduler_config.json` dict -> DDPMScheduler.  Accepted: beta_schedule scaled_linear / linear,
        beta_start, beta_end, num_train_timesteps, prediction_type epsilon / v_prediction, clip_sample false.  Raises on
        anything this class would not reproduce exactly (trained_betas, clip_sample true, thresholding,
        rescale_betas_zero_snr, another prediction_type or beta_schedule); keys that do not affect x0 are ignored."""
        c = dict(config)
        bad = []
        if c.get('trained_betas') is not None:
            bad.append('trained_betas')
        if c.get('clip_sample', False):
            bad.append('clip_sample=true')
        if c.get('thresholding', False):
            bad.append('thresholding=true')
        if c.get('rescale_betas_zero_snr', False):
            bad.append('rescale_betas_zero_snr=true')
        pt = c.get('prediction_type', 'epsilon')
        if pt not in PREDICTION_TYPES:
            bad.append(f'prediction_type={pt!r}')
        bs = c.get('beta_schedule', 'linear')       # diffusers' own default
        if bs not in ('scaled_linear', 'linear'):
            bad.append(f'beta_schedule={bs!r}')
        if bad:
            raise ValueError(f'scheduler config not supported: {", ".join(bad)}')
        kw = dict(prediction_type=pt, beta_schedule=bs)
        for k in ('num_train_timesteps', 'beta_start', 'beta_end'):
            if k in c:
                kw[k] = c[k]
        return cls(**kw)

    def to(self, device):
        for k in ('betas', 'alphas_cumprod', '_s0', '_s1', '_w'):
            setattr(self, k, getattr(self, k).to(device))
        return self

    def __repr__(self):
        return f'DDPMScheduler({self.config.beta_schedule}, {self.config.num_train_timesteps} steps, {self.config.prediction_type})'

    @property
    def mode(self):
        """sidlsg_cfg_x0 mode of this parameterisation (1 epsilon, 2 v)."""
        return prediction_mode(self.config.prediction_type)

    def coefficients(self, t):
        if self._s0.device != t.device:
            self.to(t.device)
        t = t.reshape(-1)
        return self._s0[t].contiguous(), self._s1[t].contiguous()

    def snr_weights(self, t):
        """Per-sample weight w = snr/(snr+1), snr = abar/(1-abar) (diffusers' compute_snr), of the v fake-score loss."""
        if self._w.device != t.device:
            self.to(t.device)
        return self._w[t.reshape(-1)].contiguous()

    # ---- generic duck-typed API (plain tensor math; used with non-HIP networks and on the cold path)
    def add_noise(self, original_samples, noise, timesteps):
        s0, s1 = self.coefficients(timesteps.to(original_samples.device))
        shape = (-1,) + (1,) * (original_samples.ndim - 1)
        return s0.to(original_samples.dtype).view(shape) * original_samples + s1.to(noise.dtype).view(shape) * noise

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, return_dict=True):
        t = timestep if torch.is_tensor(timestep) else torch.tensor(timestep)
        s0, s1 = self.coefficients(t.to(sample.device))
        s0, s1 = s0.to(sample.dtype), s1.to(sample.dtype)
        if s0.numel() > 1:
            shape = (-1,) + (1,) * (sample.ndim - 1)
            s0, s1 = s0.view(shape), s1.view(shape)
        if self.config.prediction_type == 'v_prediction':
            return SimpleNamespace(pred_original_sample=s0 * sample - s1 * model_output)
        return SimpleNamespace(pred_original_sample=(sample - s1 * model_output) / s0)

    def get_velocity(self, sample, noise, timesteps):
        s0, s1 = self.coefficients(timesteps.to(sample.device))
        shape = (-1,) + (1,) * (sample.ndim - 1)
        return s0.view(shape) * noise - s1.view(shape) * sample
