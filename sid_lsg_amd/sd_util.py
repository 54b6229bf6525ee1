"""SD glue with the reference's names and signatures (training/sid_sd_util.py):
    load_sd15        :51-118   -> (unet, vae, noise_scheduler, text_encoder, tokenizer)
    sid_sd_sampler   :163-211  one-step (or few-step) generator  z -> x_hat (or decoded images); the N-step training
                               sampler is hip_generate_steps (one sidlsg_step_renoise launch per step boundary)
    sid_sd_denoise   :214-274  add_noise -> (CFG-batched) UNet -> guided eps or x0 prediction
    teacher_sample   (no counterpart: the reference's tables take the teacher row from diffusers' pipeline)  guided N-step DDIM
                               sampling of the teacher itself, one sidlsg_ddim_step launch per step boundary
    teacher_sample_solver  (no counterpart)  the same under DPM-Solver++ 2M or DDIM with any eta, 'leading' / 'trailing' / 'linspace'
                               spacing and guidance rescale, one sidlsg_solver_step launch per step boundary
    teacher_sample_i2i / teacher_sample_solver_i2i  (no counterpart)  the two above entered in the middle of their chain from encoded
                               init latents (image-to-image) and, with a mask, inpainting: one sidlsg_masked_renoise launch per step
                               boundary re-imposes the kept region; sid_sd_sampler(mask=...) does the same for a distilled generator

`unet` must be a HipUNet2DCondition (bare or wrapped in DistributedDataParallel, as the reference's loop passes it):
the whole glue runs as fused HIP kernels (sidlsg_noisy_input / UNet / sidlsg_cfg_x0: no per-sample python loop, no
host syncs, the CFG pair [uncond ; cond] shares one x_t).  There is no generic / CPU branch: any other network raises.
"""
import os
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import ops
from .scheduler import SD_SAMPLING_CONFIG, DDPMScheduler, ddim_schedule, solver_schedule
from .text import TEXT_CONFIGS, CLIPBPETokenizer, CLIPTextModel, HashTokenizer, HipCLIPTextModel, resolve_text_encoder
from .unet import CONFIGS, HipUNet2DCondition


TEACHER = 'teacher'                    # value of --network / --network_pkl that stands for the teacher of the model itself
TEACHER_STEPS, TEACHER_CFG = 50, 7.5   # its default DDIM step count and guidance scale (teacher_sample, both command lines)


def _unwrap(net):
    return net.module if hasattr(net, 'module') and isinstance(net.module, torch.nn.Module) else net


def _ddp_exchange(net, out):
    """INTEGRATION.md mode 2: the reference wraps fake_score / G in DistributedDataParallel (sid_training_loop.py:316-323)
    and hands the WRAPPER to sid_sd_sampler / sid_sd_denoise.  The HIP networks accumulate weight gradients in place in
    one flat buffer (autograd never sees per-parameter gradients), so DDP's bucket hooks cannot fire; the wrapper is
    honoured as a marker instead: when it is in sync mode (outside `no_sync()`, i.e. the last accumulation round of
    misc.ddp_sync, torch_utils/misc.py:168-175) the flat gradient buffer is all-reduced to the mean once this backward
    pass has finished -- the same result DDP's buckets produce, as one exchange."""
    inner = _unwrap(net)
    if inner is net or not (torch.distributed.is_available() and torch.distributed.is_initialized()):
        return out
    world = torch.distributed.get_world_size()
    if world == 1 or not getattr(net, 'require_backward_grad_sync', True) or not inner._train_params:
        return out

    def exchange():
        # engine callbacks run in FIFO order and this one was queued by the FIRST node of the backward, i.e. before the
        # weight-gradient stream's own join callback (armed at the first wgrad launch): wait for that stream here
        g = inner.flat_grads
        ops.flush_deferred()          # queued dgamma / dbeta reductions first (their own end-of-backward callback may run after this one)
        if g.is_cuda:
            cur = torch.cuda.current_stream(g.device)
            for s in ops.grad_streams(g.device):
                cur.wait_stream(s)
        torch.distributed.all_reduce(g)
        g.div_(world)
    return ops.after_backward(out, exchange)


def _is_hip(net):
    return isinstance(_unwrap(net), HipUNet2DCondition)


def _require_hip(net):
    """The glue below drives the HIP kernels directly (NHWC bf16, fused scheduler arithmetic).  It has no generic /
    CPU branch: a foreign UNet belongs with the reference's own sid_sd_util (mode 2)."""
    if not _is_hip(net):
        raise TypeError(f'sid_lsg_amd.sd_util works on HipUNet2DCondition networks only, got {type(_unwrap(net)).__name__}')


def _arch_from_dir(path):
    """Architecture of a local diffusers-layout directory from its unet/config.json (block_out_channels,
    cross_attention_dim, use_linear_projection -- the fields that distinguish the supported configurations)."""
    import json
    cj = os.path.join(path, 'unet', 'config.json')
    if not os.path.isfile(cj):
        return None
    c = json.load(open(cj))
    for name, cfg in CONFIGS.items():
        if (tuple(c.get('block_out_channels', ())) == tuple(cfg.block_out_channels) and c.get('cross_attention_dim') == cfg.cross_attention_dim
                and bool(c.get('use_linear_projection', False)) == cfg.use_linear_projection):
            return name
    raise ValueError(f'{cj}: not one of the supported UNet configurations {sorted(CONFIGS)}')


def _random_spec(name):
    """'random:<arch>[:v]' -> (arch, prediction_type or None)."""
    parts = name.lower().split(':')
    if len(parts) == 3 and parts[2] == 'v':
        return parts[1], 'v_prediction'
    if len(parts) != 2:
        raise ValueError(f"{name}: expected 'random:<arch>' or 'random:<arch>:v'")
    return parts[1], None


def _arch_of(name):
    if os.path.isdir(name):
        arch = _arch_from_dir(name)
        if arch is not None:
            return arch
    n = os.path.basename(os.path.normpath(name)).lower() if os.path.isdir(name) else name.lower()
    if n.startswith('random:'):
        return _random_spec(n)[0]
    if '2-1-base' in n or 'sd21' in n or 'stable-diffusion-2' in n:
        return 'sd21-base'
    return 'sd15'


def resolve_scheduler(name):
    """The noise scheduler of a model spec (what load_sd15 returns, on the CPU):
      * a local diffusers-layout directory with scheduler/scheduler_config.json -> DDPMScheduler.from_config of that file
        (prediction_type epsilon or v_prediction; anything it would not reproduce exactly raises);
      * 'random:<arch>:v' -> v-prediction; 'random:<arch>' -> epsilon;
      * with SIDLSG_ALLOW_RANDOM_INIT=1, the SD 2.x hub ids WITHOUT '-base' (stable-diffusion-2-1, stable-diffusion-2: the 768-v
        checkpoints) -> v-prediction;
      * otherwise today's default (scaled_linear 0.00085..0.012, 1000 steps, epsilon)."""
    sched, sampling = _resolve_scheduler(str(name))
    sched.sampling_config = sampling
    return sched


def _resolve_scheduler(name):
    """-> (DDPMScheduler, sampling config).  The sampling config is what teacher_sample's DDIM schedule reads (steps_offset,
    set_alpha_to_one, timestep_spacing): the keys of the model's scheduler_config.json when there is one (diffusers' defaults for
    the absent ones), else the values of the SD 1.x / 2.x files."""
    import json
    if os.path.isdir(name):
        sj = os.path.join(name, 'scheduler', 'scheduler_config.json')
        if os.path.isfile(sj):
            with open(sj) as f:
                c = json.load(f)
            return DDPMScheduler.from_config(c), {k: c[k] for k in SD_SAMPLING_CONFIG if k in c}
        return DDPMScheduler(), dict(SD_SAMPLING_CONFIG)
    n = name.lower()
    if n.startswith('random:'):
        pt = _random_spec(n)[1]
        return DDPMScheduler(prediction_type=pt or 'epsilon'), dict(SD_SAMPLING_CONFIG)
    if os.environ.get('SIDLSG_ALLOW_RANDOM_INIT', '0') == '1':
        base = n.rstrip('/').rsplit('/', 1)[-1]
        if base in ('stable-diffusion-2-1', 'stable-diffusion-2'):
            return DDPMScheduler(prediction_type='v_prediction'), dict(SD_SAMPLING_CONFIG)
    return DDPMScheduler(), dict(SD_SAMPLING_CONFIG)


def check_prediction_type(unet, noise_scheduler):
    """A network trained for one parameterisation evaluated under a scheduler of the other would be read wrongly without a
    trace (e.g. a v snapshot sampled with an epsilon --repo_id): refuse."""
    net_pt = getattr(_unwrap(unet), 'prediction_type', 'epsilon')
    sch_pt = noise_scheduler.config.prediction_type
    if net_pt != sch_pt:
        raise ValueError(f'the network predicts {net_pt!r} but the noise scheduler is configured for {sch_pt!r}: '
                         'use the scheduler of the model the network was distilled from')


def resolve_compute_dtype(compute_dtype=None):
    if compute_dtype is None:
        compute_dtype = os.environ.get('SIDLSG_COMPUTE_DTYPE', 'bf16')
    if isinstance(compute_dtype, str):
        try:
            compute_dtype = {'bf16': torch.bfloat16, 'bfloat16': torch.bfloat16, 'fp32': torch.float32, 'float32': torch.float32}[compute_dtype.lower()]
        except KeyError:
            raise ValueError(f'compute dtype {compute_dtype!r}: expected bf16 or fp32') from None
    return compute_dtype


def load_sd15(pretrained_model_name_or_path, pretrained_vae_model_name_or_path, device, weight_dtype, revision=None,
              variant=None, lora_config=None, enable_xformers=False, gradient_checkpointing=False, seed=0, compute_dtype=None, text_encoder=None):
    """Same contract as the reference factory.  Sources, in order:
      * a local diffusers-layout directory (unet/diffusion_pytorch_model.safetensors, text_encoder/model.safetensors,
        tokenizer/{vocab.json,merges.txt}) -> real weights through `load_state_dict` (key names are diffusers');
      * 'random:<arch>' (arch in sd15 | sd21-base | tiny | tiny40), or any hub id when SIDLSG_ALLOW_RANDOM_INIT=1 ->
        seeded random weights of that architecture (no network here: benchmarks and parity tests use this).
    The noise scheduler (and the `prediction_type` attribute of the returned UNet) come from resolve_scheduler:
    <dir>/scheduler/scheduler_config.json when it exists, 'random:<arch>:v' for a v-prediction spec.
    `weight_dtype` is accepted for signature compatibility (the reference passes its fp16/fp32 switch here): masters are
    always fp32.  The COMPUTE dtype is `compute_dtype` (torch.bfloat16 = production MFMA path, torch.float32 = the
    fp32-accurate mode of csrc/fp32.hip), default from $SIDLSG_COMPUTE_DTYPE ('bf16' | 'fp32'), else bf16.
    `enable_xformers` / `gradient_checkpointing` are accepted and ignored (attention is always the fused HIP kernel;
    the reference itself never forwards gradient_checkpointing, sid_training_loop.py:224-228).
    `text_encoder` (not a reference option): 'torch' = text.CLIPTextModel, the PyTorch module; 'hip' = text.HipCLIPTextModel, the same
    seeded or loaded weights on the HIP kernels; default from $SIDLSG_TEXT_ENCODER, else 'torch'."""
    text_encoder_kind = resolve_text_encoder(text_encoder)
    name = str(pretrained_model_name_or_path)
    arch = _arch_of(name)
    device = torch.device(device)
    local = os.path.isdir(name)
    if not local and not name.lower().startswith('random:') and os.environ.get('SIDLSG_ALLOW_RANDOM_INIT', '0') != '1':
        raise FileNotFoundError(f'{name}: not a local diffusers directory and there is no network; pass a directory, '
                                f"'random:{arch}', or set SIDLSG_ALLOW_RANDOM_INIT=1")
    cfg = CONFIGS[arch]
    src = None
    if local:
        from safetensors.torch import load_file
        src = load_file(os.path.join(name, 'unet', 'diffusion_pytorch_model.safetensors'))
    noise_scheduler = resolve_scheduler(name)
    unet = HipUNet2DCondition(cfg, compute_dtype=resolve_compute_dtype(compute_dtype))
    unet.prediction_type = noise_scheduler.config.prediction_type
    unet.materialize(device, seed=seed, source=src)
    tcfg = TEXT_CONFIGS.get(arch, dict(hidden=cfg.cross_attention_dim, layers=2, heads=2, dff=2 * cfg.cross_attention_dim,
                                       act='quick_gelu'))
    g = torch.random.get_rng_state()
    torch.manual_seed(seed + 1)
    text_encoder = CLIPTextModel(max_pos=cfg.text_len, **tcfg)
    torch.random.set_rng_state(g)
    tokenizer = HashTokenizer(model_max_length=cfg.text_len, pad_token_id=0 if arch == 'sd21-base' else 49407)
    if local:
        from safetensors.torch import load_file
        te = os.path.join(name, 'text_encoder', 'model.safetensors')
        if os.path.isfile(te):
            res = text_encoder.load_state_dict(load_file(te), strict=False)
            # transformers checkpoints may carry the (non-parameter) position-id buffer; anything else missing or
            # unexpected would silently leave seeded random weights in the conditioning of all three networks
            bad = [k for k in list(res.missing_keys) + list(res.unexpected_keys) if not k.endswith('position_ids')]
            if bad:
                raise RuntimeError(f'{te}: text-encoder checkpoint does not match the architecture: {bad[:8]}')
        vj, mt = os.path.join(name, 'tokenizer', 'vocab.json'), os.path.join(name, 'tokenizer', 'merges.txt')
        if os.path.isfile(vj) and os.path.isfile(mt):
            tokenizer = CLIPBPETokenizer.from_files(vj, mt, model_max_length=cfg.text_len, pad_token_id=tokenizer.pad_token_id)
    text_encoder.requires_grad_(False).eval().to(device)
    if text_encoder_kind == 'hip':
        text_encoder = HipCLIPTextModel.from_torch(text_encoder)
    # VAE (decode only; cold path): real weights when the directory has them, seeded random ones otherwise
    vae_dir = pretrained_vae_model_name_or_path if (pretrained_vae_model_name_or_path and os.path.isdir(str(pretrained_vae_model_name_or_path))) else name
    vae_file = os.path.join(str(vae_dir), 'vae', 'diffusion_pytorch_model.safetensors')
    from .vae import HipAutoencoderKLDecoder
    vae = HipAutoencoderKLDecoder('sd' if arch in ('sd15', 'sd21-base') else 'tiny')
    if local and os.path.isfile(vae_file):
        from safetensors.torch import load_file
        vae.load_state_dict(load_file(vae_file))
    else:
        vae.init_parameters(seed + 2)
    vae = vae.to(device)
    return unet, vae, noise_scheduler.to(device), text_encoder, tokenizer


def load_vae_encoder(pretrained_model_name_or_path, device, seed=0):
    """The encoder half of the model's AutoencoderKL (HipAutoencoderKLEncoder) for the same specs load_sd15 takes: a local
    diffusers-layout directory -> its vae/diffusion_pytorch_model.safetensors (the file the decoder loads its half from), 'random:<arch>'
    (or a directory without that file) -> seeded random weights.  Not part of load_sd15's tuple: only image-to-image needs it."""
    name = str(pretrained_model_name_or_path)
    arch = _arch_of(name)
    local = os.path.isdir(name)
    if not local and not name.lower().startswith('random:') and os.environ.get('SIDLSG_ALLOW_RANDOM_INIT', '0') != '1':
        raise FileNotFoundError(f"{name}: not a local diffusers directory and there is no network; pass a directory or 'random:{arch}'")
    from .vae import HipAutoencoderKLEncoder
    enc = HipAutoencoderKLEncoder('sd' if arch in ('sd15', 'sd21-base') else 'tiny')
    vae_file = os.path.join(name, 'vae', 'diffusion_pytorch_model.safetensors')
    if local and os.path.isfile(vae_file):
        from safetensors.torch import load_file
        res = enc.load_state_dict(load_file(vae_file))
        if res.missing_keys:
            raise RuntimeError(f'{vae_file}: no encoder weights for {res.missing_keys[:8]}')
    else:
        enc.init_parameters(seed + 3)
    return enc.to(torch.device(device))


def load_controlnet(spec, unet, device, seed=0):
    """A ControlNet (controlnet.HipControlNet) for `unet`, in its compute dtype:
      * a local directory in diffusers' layout (config.json, diffusion_pytorch_model.safetensors): the config must describe a copy of
        the UNet's encoder (block_out_channels, cross_attention_dim, use_linear_projection, heads) without global_pool_conditions,
        class_embed_type, addition_embed_type or conditioning_channels != 3; a missing key or a wrong shape is refused by name;
      * 'random:controlnet[:seed]': seeded weights of the UNet's own architecture (seed from the spec, else `seed`).
    In the seeded form the thirteen tap convolutions and the embedder's conv_out get ordinary fan-in-scaled NON-zero weights.  diffusers
    initialises them to zero, so that an untrained ControlNet changes nothing; here that would make a seeded ControlNet a no-op and every
    test of the conditioning path vacuous."""
    from . import controlnet as cn
    net = _unwrap(unet)
    _require_hip(net)
    if isinstance(net, cn.HipControlNet):
        raise TypeError('load_controlnet: `unet` is itself a ControlNet')
    name = str(spec)
    if os.path.isdir(name):
        return cn.load_controlnet_dir(name, net, torch.device(device))
    if not name.lower().startswith('random:'):
        raise FileNotFoundError(f"{name}: not a local ControlNet directory; pass a directory or '{cn.RANDOM_PREFIX}[:seed]'")
    s = cn.parse_random_spec(name)
    return cn.HipControlNet(net.cfg, compute_dtype=net.compute_dtype).materialize(torch.device(device), seed=seed if s is None else s)


def load_ip_adapter(spec, unet, device, embed_dim, seed=0):
    """An IP-Adapter (ip_adapter.HipIPAdapter) for `unet`, in its compute dtype, for an image encoder of projection_dim `embed_dim`: a
    local `.safetensors` / `.bin` file in the published layout or 'random:ip-adapter[:seed]' (ip_adapter.load_ip_adapter)."""
    from . import ip_adapter as ipa
    net = _unwrap(unet)
    _require_hip(net)
    return ipa.load_ip_adapter(spec, net, torch.device(device), embed_dim, seed=seed)


def lora_scales(nfiles, scales):
    """The --lora_scale rule of both command lines: no value -> 1 for every file, one value -> that for every file, else one per file."""
    scales = [float(s) for s in (scales or ())]
    if nfiles == 0:
        if scales:
            raise ValueError('--lora_scale applies to --lora only')
        return []
    if len(scales) not in (0, 1, nfiles):
        raise ValueError(f'{len(scales)} --lora_scale values for {nfiles} --lora files: give none, one, or one per file')
    return [1.0] * nfiles if not scales else scales * nfiles if len(scales) == 1 else scales


def load_lora(specs, scales, unet, text_encoder=None, seed=0, log=print):
    """LoRA files ATTACHED to `unet` and `text_encoder` (lora.LoraSet; one merge launch per network, then the refresh): each spec is a
    local kohya / diffusers `.safetensors` / `.bin` / `.pt` file or 'random:lora[:rank[:seed]]'; `scales` one per spec.  Prints one line
    per file through `log` and returns the LoraSet (`set_scales`, `detach`)."""
    from . import lora
    net = _unwrap(unet)
    _require_hip(net)
    adapters, notes = lora.load_adapters(specs, net, text_encoder, seed=seed)
    for note in notes:
        log(note)
    ls = lora.LoraSet(net, text_encoder).attach(adapters, scales)
    for spec, s, (nu, nt, r0, r1) in zip(specs, scales, lora.summary(adapters)):
        log(f'LoRA "{spec}": {nu} UNet + {nt} text-encoder layers, rank {r0 if r0 == r1 else f"{r0}-{r1}"}, scale {float(s):g}')
    return ls


def encode_contexts(contexts, text_encoder, tokenizer, device):
    """list[str] -> [B, L, D] text states (no grad); a tensor is passed through (pre-computed states)."""
    if torch.is_tensor(contexts):
        return contexts
    ids = tokenizer(list(contexts), padding='max_length', max_length=tokenizer.model_max_length, truncation=True,
                    return_tensors='pt').input_ids
    with torch.no_grad():
        return text_encoder(ids.to(device))[0]


# ------------------------------------------------------------------------------------------------
def hip_generate(unet, z, ctx16, init_t, sched, x0=None, control=None, ip=None):
    """x_t = s0*x0 + s1*z at t_init ; o = G(x_t) ; x_hat = (x_t - s1*o)/s0 (epsilon) or s0*x_t - s1*o (v)   (sid_sd_util.py:182-185)"""
    s0, s1 = sched.coefficients(init_t)
    net = _unwrap(unet)
    xin, xt = ops.noisy_input(x0, z, s0, s1, 1, net.compute_dtype)
    eps = _ddp_exchange(unet, net.forward_nhwc(xin, init_t, ctx16, control=control, ip=ip))
    return ops.cfg_x0(eps, xt, s0, s1, 1.0, True, net.compute_dtype, prediction_type=sched.config.prediction_type)


def step_timesteps(init_t, num_steps):
    """t_i = (init_t * (1 - i/N)).long() for i < N: float arithmetic, then truncation (sid_sd_util.py:178)."""
    return [(init_t * (1 - i / num_steps)).to(torch.long) for i in range(num_steps)]


def hip_generate_steps(unet, z, eps_next, ctx16, init_t, sched):
    """The N-step generator of the reference's training sampler (sid_sd_util.py:176-185), N = 1 + len(eps_next):
    x_{t_0} = s1 z; for each step x_hat_i = x0 prediction of G(x_{t_i}, t_i); x_{t_{i+1}} = add_noise(x_hat_i, eps_next[i], t_{i+1}).
    eps_next: [N-1, B, 4, h, w] fp32 (the eps_1 .. eps_{N-1} the caller drew), or None: one step = hip_generate, same launches.
    Each step boundary is one sidlsg_step_renoise launch each way; the last x_hat comes from cfg_x0.
    Only the step-0 forward of G places gradient-exchange markers (set_grad_ready_callback) and the mode-2 exchange: its backward
    is the last one to add to G's weight gradients, so a segment is final only once step 0's backward has passed it."""
    if eps_next is None or len(eps_next) == 0:
        return hip_generate(unet, z, ctx16, init_t, sched)
    net = _unwrap(unet)
    if torch.is_grad_enabled() and net._train_params and ops.wgrad_stream_count() > 1:
        raise RuntimeError('multi-step generator training with SIDLSG_WGRAD_STREAMS > 1: the N weight gradients of one layer would '
                           'land on different weight-gradient streams unordered; use SIDLSG_WGRAD_STREAMS=1')
    n = len(eps_next) + 1
    pt, dt = sched.config.prediction_type, net.compute_dtype
    ts = step_timesteps(init_t, n)
    s0, s1 = sched.coefficients(ts[0])
    xin, xt = ops.noisy_input(None, z, s0, s1, 1, dt)
    cb = net._grad_ready_cb
    try:
        for i in range(n):
            eps = net.forward_nhwc(xin, ts[i], ctx16)
            if i == 0:
                eps = _ddp_exchange(unet, eps)
                net._grad_ready_cb = None
            if i == n - 1:
                return ops.cfg_x0(eps, xt, s0, s1, 1.0, True, dt, prediction_type=pt)
            s0n, s1n = sched.coefficients(ts[i + 1])
            xin, xt = ops.step_renoise(eps, xt, s0, s1, s0n, s1n, eps_next[i], dt, prediction_type=pt)
            s0, s1 = s0n, s1n
    finally:
        net._grad_ready_cb = cb


def hip_prepare_denoise(images, noise, t, cond16, uncond16, sched, guided, act_dtype=torch.bfloat16):
    """Shared by every network evaluated on the same (images, noise, t): the noisy CFG batch and its conditioning
    (`act_dtype` = the compute dtype of the networks that will consume it)."""
    s0, s1 = sched.coefficients(t)
    dup = 2 if guided else 1
    xin, xt = ops.noisy_input(images, noise, s0, s1, dup, act_dtype)
    ctx = torch.cat([uncond16, cond16]) if guided else cond16          # (sid_sd_util.py:259-261)
    tt = torch.cat([t, t]) if guided else t
    return SimpleNamespace(xin=xin, xt=xt, s0=s0, s1=s1, ctx=ctx, tt=tt, prediction_type=sched.config.prediction_type)


def hip_denoise(unet, prep, guidance_scale, predict_x0):
    net = _unwrap(unet)
    eps = _ddp_exchange(unet, net.forward_nhwc(prep.xin, prep.tt, prep.ctx))
    return ops.cfg_x0(eps, prep.xt, prep.s0, prep.s1, guidance_scale, predict_x0, net.compute_dtype,     # u + k(c-u), then x0 (:264-272)
                      prediction_type=prep.prediction_type)


# ------------------------------------------------------------------------------------------------
def sid_sd_sampler(unet, latents, contexts, init_timesteps, noise_scheduler, text_encoder, tokenizer, resolution,
                   dtype=torch.float16, return_images=False, vae=None, guidance_scale=1, num_steps=1, train_sampler=True,
                   num_steps_eval=1, init_latents=None, start_step=0, mask=None, control=None, ip=None):
    """ip (eval mode only): an ip_adapter.IPState (HipIPAdapter.prepare(image_embeds, scale, dup=1)), passed to every UNet call of the loop;
    it composes with control.
    control (eval mode only): a controlnet.ControlState (HipControlNet.prepare(images, scale, dup=1)), passed to every UNet call of the loop.
    init_latents / start_step (eval mode only; image-to-image): the chain is entered at step `start_step` with D_x = init_latents
    (scaled latents [B, 4, h, w], e.g. HipAutoencoderKLEncoder.encode_latents); the first executed step takes `latents` as its noise,
    so its input is x_{t_k} = s0 init_latents + s1 latents -- what a generator trained with --num_steps N saw at step k.
    mask (eval mode only, needs init_latents; inpainting): uint8 / bool [B, h, w] or [1, h, w], nonzero = repaint.  After every
    executed step's x0 prediction D_x <- mask ? D_x : init_latents (one sidlsg_masked_renoise launch, a select); the next step noises
    the kept region to its level with its own noise."""
    steps = num_steps if train_sampler else num_steps_eval
    if init_latents is None:
        if start_step != 0:
            raise ValueError('sid_sd_sampler: start_step without init_latents')
    elif train_sampler:
        raise ValueError('sid_sd_sampler: init_latents is for the evaluation sampler (train_sampler=False)')
    elif not 0 <= start_step < steps:
        raise ValueError(f'sid_sd_sampler: start_step {start_step} outside [0, {steps})')
    elif init_latents.shape != latents.shape:
        raise ValueError(f'sid_sd_sampler: init_latents {tuple(init_latents.shape)} vs latents {tuple(latents.shape)}')
    if mask is not None:
        if train_sampler:
            raise ValueError('sid_sd_sampler: mask is for the evaluation sampler (train_sampler=False)')
        mask = check_mask(mask, init_latents, latents, 'sid_sd_sampler')
    if control is not None and train_sampler:
        raise ValueError('sid_sd_sampler: control is for the evaluation sampler (train_sampler=False): ControlNet conditioning is forward only')
    if ip is not None and train_sampler:
        raise ValueError('sid_sd_sampler: ip is for the evaluation sampler (train_sampler=False): IP-Adapter conditioning is forward only')
    _require_hip(unet)
    check_prediction_type(unet, noise_scheduler)
    emb = encode_contexts(contexts, text_encoder, tokenizer, latents.device).to(_unwrap(unet).compute_dtype).contiguous()
    D_x = None
    ctxmgr = torch.enable_grad() if train_sampler else torch.no_grad()
    with ctxmgr:
        if train_sampler and steps > 1:
            # the eps_i the reference draws between its steps (randn_like, :179), drawn up front: the steps consume no RNG
            eps_next = torch.stack([torch.randn_like(latents) for _ in range(steps - 1)]).to(torch.float32).contiguous()
            D_x = hip_generate_steps(unet, latents.to(torch.float32).contiguous(), eps_next, emb, init_timesteps.contiguous(),
                                     noise_scheduler)
        else:
            if init_latents is not None:
                D_x = z0 = init_latents.to(torch.float32).contiguous()
            for i in range(start_step, steps):
                noise = latents if i == start_step else torch.randn_like(latents)
                t_i = (init_timesteps * (1 - i / steps)).to(torch.long)
                D_x = hip_generate(unet, noise.to(torch.float32).contiguous(), emb, t_i.contiguous(), noise_scheduler, x0=D_x, control=control, ip=ip)
                if mask is not None:
                    D_x = ops.masked_renoise(D_x, z0, mask, want_input=False, inplace=True)[1]
    return decode_latents(vae, D_x) if return_images else D_x.to(torch.float32)


def decode_latents(vae, x):
    """Scaled latents -> images fp32: vae.decode(x / scaling_factor), a float16 VAE with force_upcast run in float32 for the call."""
    upcast = vae.dtype == torch.float16 and getattr(vae.config, 'force_upcast', False)
    if upcast:
        vae.to(dtype=torch.float32)
    images = vae.decode(x.to(vae.dtype) / vae.config.scaling_factor, return_dict=False)[0]
    if upcast:
        vae.to(dtype=torch.float16)
    return images.to(torch.float32)


def sid_sd_denoise(unet, images, noise, contexts, timesteps, noise_scheduler, text_encoder, tokenizer, resolution,
                   dtype=torch.float16, predict_x0=True, guidance_scale=1):
    _require_hip(unet)
    check_prediction_type(unet, noise_scheduler)
    b = images.shape[0]
    cond = encode_contexts(contexts, text_encoder, tokenizer, images.device)
    guided = guidance_scale != 1
    uncond = encode_contexts([''] * b, text_encoder, tokenizer, images.device) if guided else None
    bf = _unwrap(unet).compute_dtype
    prep = hip_prepare_denoise(images.to(torch.float32).contiguous(), noise.to(torch.float32).contiguous(),
                               timesteps.contiguous(), cond.to(bf).contiguous(),
                               uncond.to(bf).contiguous() if guided else None, noise_scheduler, guided, act_dtype=bf)
    return hip_denoise(unet, prep, float(guidance_scale), predict_x0)


def teacher_start_index(num_inference_steps, strength):
    """Image-to-image entry of an N-step teacher sampler at `strength` S: run = min(int(N*S), N) steps are executed, the steps
    k .. N-1 with k = N - run -- a restatement of diffusers' StableDiffusionImg2ImgPipeline.get_timesteps, N*S formed in floating
    point as there (int(10*0.3) == 3, int(100*0.29) == 28).  -> k; fewer than one executed step is a ValueError."""
    n = int(num_inference_steps)
    if n < 1:
        raise ValueError(f'num_inference_steps={n}: expected at least 1')
    run = min(int(n * strength), n)
    if run < 1:
        raise ValueError(f'strength={strength}: int({n}*{strength}) = {run} of the {n} steps would run; expected at least 1')
    return n - run


def check_mask(mask, init_latents, latents, who):
    """An inpainting mask (uint8 / bool [B, h, w] or [1, h, w], nonzero = repaint) for latents [B, C, h, w] -> contiguous, on their
    device.  A mask needs init_latents: they are the known region."""
    if init_latents is None:
        raise ValueError(f'{who}: mask without init_latents (they are the region that is kept)')
    b, _, h, w = latents.shape
    if not torch.is_tensor(mask) or mask.dtype not in (torch.uint8, torch.bool) or mask.dim() != 3 or mask.shape[0] not in (1, b) \
            or tuple(mask.shape[1:]) != (h, w):
        got = f'{tuple(mask.shape)} {mask.dtype}' if torch.is_tensor(mask) else type(mask).__name__
        raise ValueError(f'{who}: mask {got}: expected uint8 or bool [{b} or 1, {h}, {w}]')
    return mask.to(latents.device).contiguous()


def _teacher_entry(latents, init_latents, start_index, mask, n, who):
    """The image-to-image / inpainting arguments of the teacher samplers, checked -> (z0 fp32 or None, mask or None, noised start?).
    The start state is alpha_k*z0 + sigma_k*z, except with a mask at k = 0 (diffusers' is_strength_max): pure noise, as without init."""
    if init_latents is None:
        if start_index != 0:
            raise ValueError(f'{who}: start_index without init_latents')
        if mask is not None:
            check_mask(mask, init_latents, latents, who)
        return None, None, False
    if not 0 <= start_index < n:
        raise ValueError(f'{who}: start_index {start_index} outside [0, {n})')
    if init_latents.shape != latents.shape:
        raise ValueError(f'{who}: init_latents {tuple(init_latents.shape)} vs latents {tuple(latents.shape)}')
    if mask is not None:
        mask = check_mask(mask, init_latents, latents, who)
    return init_latents.to(torch.float32).contiguous(), mask, not (mask is not None and start_index == 0)


def sampling_config_of(noise_scheduler, schedule_config=None):
    """The DDIM sampling keys teacher_sample uses: `schedule_config` when given, else what resolve_scheduler attached to the scheduler
    (an EMPTY dict there means a scheduler_config.json without these keys, i.e. diffusers' defaults), else the SD values."""
    if schedule_config is not None:
        return schedule_config
    found = getattr(noise_scheduler, 'sampling_config', None)
    return SD_SAMPLING_CONFIG if found is None else found


def _teacher_loop(who, plan, unet, latents, contexts, negative_contexts, noise_scheduler, text_encoder, tokenizer, guidance_scale, return_images,
                  vae, init_latents, start_index, mask, control, ip):
    """The loop under teacher_sample_i2i and teacher_sample_solver_i2i.  `plan(z, compute dtype, prediction type, entry)` is the sampler's
    part: it builds its tables on z's device, calls `entry(n)` (_teacher_entry) once, and returns (what entry returned, ts [n], s0 [n, b],
    s1 [n, b], step, renoise) with `step(i, eps, x_t, last) -> (next network input, x_prev)` the boundary launch(es) of step i and
    `renoise(i) -> (a0, a1)` the level to which a mask re-noises the known region after step i.  Pinned by tests and by the files written:
      * launches: one noisy_input; per step one forward_nhwc, then the boundary (ddim_step; or cfg_rescale_stats where guided and phi != 0,
        then solver_step), then with a mask one masked_renoise (after the last step with want_input=False: z0 itself);
      * random draws: the solver boundary calls randn once per step whose c_n is non-zero, in step order, and never otherwise;
      * table casts: the DDIM plan casts its tables with .to(torch.float32) before the expand to [n, b], the solver plan does not;
      * last flag: the boundary gets last = (last step) or (mask given); start: noisy_input(None, z, ones, ones) unless `noised`;
      * error precedence: guidance_rescale's range, then _teacher_entry with int(num_inference_steps), then the schedule (solver); the
        schedule, then _teacher_entry with ts.numel() (DDIM); the length of negative_contexts after either; `who` names the public sampler."""
    _require_hip(unet)
    check_prediction_type(unet, noise_scheduler)
    net = _unwrap(unet)
    dt = net.compute_dtype
    with torch.no_grad():
        z = latents.to(torch.float32).contiguous()
        b, dev = z.shape[0], z.device
        (z0, mask, noised), ts, s0, s1, step, renoise = plan(z, dt, noise_scheduler.config.prediction_type,
                                                             lambda n: _teacher_entry(z, init_latents, start_index, mask, n, who))
        n = ts.numel()
        guided = guidance_scale != 1
        dup = 2 if guided else 1
        if negative_contexts is not None and not torch.is_tensor(negative_contexts) and len(negative_contexts) != b:
            raise ValueError(f'negative_contexts: {len(negative_contexts)} prompts for a batch of {b}')
        ctx = encode_contexts(contexts, text_encoder, tokenizer, dev).to(dt)
        if guided:
            neg = [''] * b if negative_contexts is None else negative_contexts
            ctx = torch.cat([encode_contexts(neg, text_encoder, tokenizer, dev).to(dt), ctx])
        ctx = ctx.contiguous()
        tt = ts[:, None].expand(n, dup * b).contiguous()
        ones = torch.ones(b, device=dev, dtype=torch.float32)
        if noised:
            xin, xt = ops.noisy_input(z0, z, s0[start_index], s1[start_index], dup, dt)      # x_{t_k} = alpha_k z0 + sigma_k z
        else:
            xin, xt = ops.noisy_input(None, z, ones, ones, dup, dt)      # x_T = z, as the [uncond ; cond] NHWC batch
        for i in range(start_index, n):
            eps = net.forward_nhwc(xin, tt[i], ctx, control=control, ip=ip)
            last = i == n - 1
            xin, xt = step(i, eps, xt, last or mask is not None)
            if mask is not None and last:
                xt = ops.masked_renoise(xt, z0, mask, want_input=False, inplace=True)[1]
            elif mask is not None:
                a0, a1 = renoise(i)
                xin, xt = ops.masked_renoise(xt, z0, mask, noise=z, a0=a0, a1=a1, dup=dup, act_dtype=dt, inplace=True)
        return decode_latents(vae, xt) if return_images else xt


def teacher_sample(unet, latents, contexts, noise_scheduler, text_encoder, tokenizer, resolution, guidance_scale=TEACHER_CFG,
                   num_inference_steps=TEACHER_STEPS, return_images=False, vae=None, schedule_config=None):
    """teacher_sample_i2i from pure noise: the text-to-image teacher row, under the signature it has always had."""
    return teacher_sample_i2i(unet, latents, contexts, noise_scheduler, text_encoder, tokenizer, resolution, guidance_scale=guidance_scale,
                              num_inference_steps=num_inference_steps, return_images=return_images, vae=vae, schedule_config=schedule_config)


def teacher_sample_i2i(unet, latents, contexts, noise_scheduler, text_encoder, tokenizer, resolution, guidance_scale=TEACHER_CFG,
                       num_inference_steps=TEACHER_STEPS, return_images=False, vae=None, schedule_config=None, init_latents=None,
                       start_index=0, mask=None, control=None, ip=None):
    """The teacher itself, sampled the way every SiD-LSG table samples it: classifier-free guidance and an N-step deterministic DDIM
    sampler (Song et al. 2021, eta = 0; diffusers' DDIMScheduler with 'leading' spacing).  x_T = latents (DDIM's init_noise_sigma is
    1); per step one UNet pass on the stacked [uncond ; cond] batch (unconditional prompt '', as sid_sd_denoise) and one
    sidlsg_ddim_step launch; guidance_scale == 1 makes no unconditional pass.  Timesteps and coefficients are device tensors indexed
    by the step number: the loop issues device work only.  `schedule_config`: the sampling keys of the model's scheduler_config.json
    (scheduler.ddim_schedule); None = what resolve_scheduler found for the model, else the SD values (sampling_config_of).
    `resolution` is accepted for the signature of the other samplers and not used: the size is the latents'.  The scheduler is not
    moved: the N-entry tables are built where it lives and copied to the latents' device before the loop.
    init_latents / start_index (image-to-image): scaled latents z0 [B, 4, h, w]; the chain is entered at step k = start_index
    (teacher_start_index) from x_{t_k} = alpha_k*z0 + sigma_k*latents, one noisy_input launch, and steps k .. N-1 run.
    mask (inpainting, needs init_latents): uint8 / bool [B, h, w] or [1, h, w], nonzero = repaint.  After every step one
    sidlsg_masked_renoise launch re-imposes the known region at the step's target level, x <- mask ? x : s0p_i*z0 + s1p_i*latents
    (after the last step: z0 itself), and writes the next network input; with a mask and k = 0 the start is pure noise (diffusers'
    is_strength_max).  These rules restate diffusers' img2img / inpainting pipelines; agreement with the package is not pinned by a test.
    control: a controlnet.ControlState (HipControlNet.prepare(images, scale, dup=2 with guidance, else 1)), passed to every UNet call; it
    composes with init_latents / start_index / mask and needs none of them (teacher_sample keeps its pinned signature: the argument lives here).
    ip: an ip_adapter.IPState (HipIPAdapter.prepare(image_embeds, scale, dup=2 with guidance, else 1)), passed to every UNet call; it
    composes with control and with the image-to-image arguments in the same way.
    -> the final latent x_0 fp32 NCHW, or (return_images) the decoded images as sid_sd_sampler returns them."""
    def plan(z, dt, pt, entry):
        ts, *tables = (v.to(z.device) for v in ddim_schedule(noise_scheduler, sampling_config_of(noise_scheduler, schedule_config), num_inference_steps))
        start = entry(ts.numel())
        s0, s1, s0p, s1p = (v.to(torch.float32)[:, None].expand(ts.numel(), z.shape[0]).contiguous() for v in tables)

        def step(i, eps, xt, last):
            return ops.ddim_step(eps, xt, s0[i], s1[i], s0p[i], s1p[i], guidance_scale, dt, prediction_type=pt, last=last)[:2]
        return start, ts, s0, s1, step, lambda i: (s0p[i], s1p[i])          # the mask re-noises to the level step i has just reached
    return _teacher_loop('teacher_sample_i2i', plan, unet, latents, contexts, None, noise_scheduler, text_encoder, tokenizer, guidance_scale,
                         return_images, vae, init_latents, start_index, mask, control, ip)


def teacher_sample_solver(unet, latents, contexts, noise_scheduler, text_encoder, tokenizer, resolution, guidance_scale=TEACHER_CFG,
                          num_inference_steps=TEACHER_STEPS, return_images=False, vae=None, schedule_config=None, solver='dpmpp2m',
                          spacing=None, eta=0.0, guidance_rescale=0.0, negative_contexts=None, randn=None):
    """teacher_sample_solver_i2i from pure noise: the text-to-image solver rows, under the signature they have always had."""
    return teacher_sample_solver_i2i(unet, latents, contexts, noise_scheduler, text_encoder, tokenizer, resolution,
                                     guidance_scale=guidance_scale, num_inference_steps=num_inference_steps, return_images=return_images,
                                     vae=vae, schedule_config=schedule_config, solver=solver, spacing=spacing, eta=eta,
                                     guidance_rescale=guidance_rescale, negative_contexts=negative_contexts, randn=randn)


def teacher_sample_solver_i2i(unet, latents, contexts, noise_scheduler, text_encoder, tokenizer, resolution, guidance_scale=TEACHER_CFG,
                              num_inference_steps=TEACHER_STEPS, return_images=False, vae=None, schedule_config=None, solver='dpmpp2m',
                              spacing=None, eta=0.0, guidance_rescale=0.0, negative_contexts=None, randn=None, init_latents=None,
                              start_index=0, mask=None, control=None, ip=None):
    """The teacher under the solvers it is usually run with: `solver` 'dpmpp2m' (DPM-Solver++ 2M) or 'ddim' (any `eta` >= 0), timestep
    `spacing` 'leading' / 'trailing' / 'linspace' (None: the model's timestep_spacing), guidance rescale `guidance_rescale` (phi of
    Lin et al. 2024; 0 = plain classifier-free guidance) and `negative_contexts` in place of '' in the unconditional half.  The
    timesteps and coefficients are scheduler.solver_schedule's.  Same loop shape as teacher_sample: contexts encoded once, x_T =
    latents, per step one UNet pass on the [uncond ; cond] batch and one sidlsg_solver_step launch (with phi != 0 and guidance, one
    sidlsg_cfg_rescale_stats launch before it), tables as device tensors indexed by the step number, the two x0 history buffers
    swapped per step: nothing waits for the device between the first UNet pass and the result.  `randn(shape) -> fp32 tensor` supplies
    xi once per step whose c_n is non-zero, in step order (default: torch.randn on the latents' device).
    init_latents / start_index / mask: image-to-image and inpainting as in teacher_sample.  The tables are solver_schedule's with
    start = start_index (DPM-Solver++ 2M takes its first executed step at first order); the masked boundary of step i noises the known
    region to the level of t_{i+1}, known = s0[i+1]*z0 + s1[i+1]*latents (after the last step: z0), and leaves the x0 history alone.
    control: a controlnet.ControlState, ip: an ip_adapter.IPState, as in teacher_sample_i2i.
    -> the final latent x_0 fp32 NCHW, or (return_images) the decoded images as sid_sd_sampler returns them."""
    def plan(z, dt, pt, entry):
        phi = float(guidance_rescale)
        if not 0 <= phi <= 1:
            raise ValueError(f'guidance_rescale={guidance_rescale}: expected a value in [0, 1]')
        start = entry(int(num_inference_steps))
        ts, s0, s1, coef = solver_schedule(noise_scheduler, sampling_config_of(noise_scheduler, schedule_config), num_inference_steps, solver=solver,
                                           spacing=spacing, eta=eta, start=start_index)
        flags = (coef.cpu() != 0).tolist()          # per step: which terms exist (read before the loop; the loop itself reads nothing back)
        ts, s0, s1, coef = (v.to(z.device) for v in (ts, s0, s1, coef))
        s0, s1 = (v[:, None].expand(ts.numel(), z.shape[0]).contiguous() for v in (s0, s1))
        coef = coef[:, None, :].expand(ts.numel(), z.shape[0], 4).contiguous()
        draw = randn if randn is not None else lambda shape: torch.randn(shape, device=z.device, dtype=torch.float32)
        history = [torch.empty_like(z), torch.empty_like(z)]          # the two x0 buffers, swapped per step
        x0_prev = None

        def step(i, eps, xt, last):
            nonlocal x0_prev
            scale = ops.cfg_rescale_stats(eps, z.shape[1], guidance_scale, phi) if guidance_scale != 1 and phi != 0 else None
            noise = draw(tuple(z.shape)).to(device=z.device, dtype=torch.float32).contiguous() if flags[i][3] else None
            xin, xt, x0_prev = ops.solver_step(eps, xt, s0[i], s1[i], coef[i], guidance_scale, dt, prediction_type=pt,
                                               x0p=x0_prev if flags[i][2] else None, noise=noise, scale=scale, last=last,
                                               x0_out=history[i & 1], need_prev=flags[i][2])
            return xin, xt
        return start, ts, s0, s1, step, lambda i: (s0[i + 1], s1[i + 1])          # the mask re-noises to the level of t_{i+1}
    return _teacher_loop('teacher_sample_solver_i2i', plan, unet, latents, contexts, negative_contexts, noise_scheduler, text_encoder, tokenizer,
                         guidance_scale, return_images, vae, init_latents, start_index, mask, control, ip)
