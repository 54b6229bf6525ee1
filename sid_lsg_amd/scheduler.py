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
