#!/usr/bin/env python
"""Command line of the distillation run, option-compatible with the reference's `sid_train.py` (boundary B5).

    torchrun --standalone --nproc_per_node=8 sid_train.py --outdir runs --data_prompt_text /data/aesthetics_6_plus \\
        --sd_model /models/stable-diffusion-v1-5 --cfg_train_fake 1.5 --cfg_eval_fake 1.5 --cfg_eval_real 1.5 \\
        --batch 64 --batch-gpu 8 --duration 10 --ema 0.05 --tick 2 --snap 50 --dump 100

Same option names, defaults and derived quantities as the reference (`sid_train.py:88-157` options, `:196-330` config):
optimizer kwargs (Adam, betas (0, 0.999), eps 1e-8 / 1e-6 under --fp16; AdamW + wd 0.01), total_kimg = duration*1000,
ema_halflife_kimg = ema*1000, run-directory numbering and description string, `--resume training-state-<kimg>.pt`.
Differences (documented, not silent):
  * `--sd_model` must be a local diffusers-layout directory or `random:<arch>` (no network in this environment);
  * `--fp16` only selects the optimizer eps; masters are fp32 and compute is bf16 MFMA, or -- with the added option
    `--precision fp32` -- the fp32-accurate mode (the reference's own default precision, ~20x slower);
  * `--deterministic 1` (added option) makes the training step bit-reproducible: same tree, GPU model, configuration and
    world size give the same bits (sid_lsg_amd.ops.set_deterministic);
  * `--snapshot_images 1` (added option) writes the preview grids `fakes_init.png` and `fakes_<alpha>_<kimg>_{1,2,4}.png` next to the
    snapshots, and `<metric><kimg>_<steps>.png` with `--train_mode 0` (sid_lsg_amd/preview.py); the reference always writes them;
  * `--metrics` run through sid_lsg_amd/metrics.py at the snapshot ticks and need a LOCAL detector file (--metric_pt_path);
    the real-set statistics come from --data_stat or, when --data is an image directory, from the images themselves (cached as
    <run_dir>/real_stats.npz); pr30k3_full / pr_test (precision / recall) always read the images;
    `--train_mode 0 --network_pkl <snapshot>` evaluates a snapshot (1 / 2 / 4 steps);
    `--train_mode 0 --network_pkl teacher` (added value) evaluates the teacher of --sd_model itself, once, under classifier-free
    guidance `--teacher_cfg` and a `--teacher_steps`-step deterministic DDIM sampler (sid_lsg_amd.sd_util.teacher_sample);
    `--teacher_sampler`, `--teacher_spacing`, `--teacher_eta`, `--teacher_rescale` choose DPM-Solver++ 2M, stochastic DDIM, another
    timestep spacing or guidance rescale instead (sid_lsg_amd.sd_util.teacher_sample_solver);
  * `--data` is optional (it is the COCO image set used only by the metrics and by reals.png).
"""
import json
import os
import re

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # dmabuf IPC for RCCL on this platform: before the HIP runtime starts

import click  # noqa: E402
import torch  # noqa: E402

from sid_lsg_amd import distributed as dist  # noqa: E402
from sid_lsg_amd.dnnlib_util import EasyDict, construct_class_by_name  # noqa: E402
from sid_lsg_amd.sd_util import TEACHER, TEACHER_CFG, TEACHER_STEPS, resolve_scheduler  # noqa: E402
from sid_lsg_amd.training_loop import training_loop  # noqa: E402


def _csv(_ctx, _param, value):
    if value is None or value == '' or value.lower() == 'none':
        return None
    return value.split(',')


# (flag(s), kwargs) -- kept as a table so that the option surface can be diffed against the reference at a glance
OPTIONS = [
    (('--outdir',), dict(type=str, required=True, metavar='DIR', help='Where to save the results')),
    (('--data',), dict(type=str, default=None, metavar='ZIP|DIR', help='Image dataset (only used by --metrics)')),
    (('--data_stat',), dict(type=str, default=None, metavar='ZIP|DIR', help='Dataset statistics (only used by --metrics)')),
    (('--data_prompt_text',), dict(type=str, required=True, metavar='DIR|TXT', help='Training prompts')),
    (('--duration',), dict(type=click.FloatRange(min=0, min_open=True), default=200, show_default=True, metavar='MIMG', help='Training duration')),
    (('--batch',), dict(type=click.IntRange(min=1), default=512, show_default=True, metavar='INT', help='Total batch size')),
    (('--batch-gpu',), dict(type=click.IntRange(min=1), default=None, metavar='INT', help='Limit batch size per GPU')),
    (('--ema',), dict(type=click.FloatRange(min=0), default=0.5, show_default=True, metavar='MIMG', help='EMA half-life')),
    (('--xflip',), dict(type=float, default=0.0, show_default=True, help='Dataset x-flips (unused by the prompt stream)')),
    (('--bench',), dict(type=bool, default=True, show_default=True, help='Accepted for compatibility (no cuDNN here)')),
    (('--cache',), dict(type=bool, default=True, show_default=True, help='Accepted for compatibility')),
    (('--workers',), dict(type=click.IntRange(min=1), default=1, show_default=True, help='Accepted for compatibility')),
    (('--desc',), dict(type=str, default=None, metavar='STR', help='String to include in result dir name')),
    (('--nosubdir',), dict(is_flag=True, help='Do not create a subdirectory for results')),
    (('--tick',), dict(type=click.IntRange(min=1), default=2, show_default=True, metavar='KIMG', help='How often to print progress')),
    (('--snap',), dict(type=click.IntRange(min=1), default=50, show_default=True, metavar='TICKS', help='How often to save snapshots')),
    (('--dump',), dict(type=click.IntRange(min=1), default=100, show_default=True, metavar='TICKS', help='How often to dump state')),
    (('--seed',), dict(type=int, default=None, metavar='INT', help='Random seed  [default: random, shared by all ranks]')),
    (('--transfer',), dict(type=str, default=None, metavar='PKL', help='Initialise G / G_ema from a network snapshot')),
    (('--resume',), dict(type=str, default=None, metavar='PT', help='Resume from training-state-*.pt')),
    (('-n', '--dry-run'), dict(is_flag=True, help='Print training options and exit')),
    (('--metrics',), dict(callback=_csv, default=None, help='Comma-separated list or "none"')),
    (('--sd_model',), dict(type=str, default='runwayml/stable-diffusion-v1-5', show_default=True, help='Local diffusers directory, random:<arch> or random:<arch>:v')),
    (('--resolution',), dict(type=int, default=512, show_default=True, metavar='INT', help='Image resolution')),
    (('--init_timestep',), dict(type=int, default=625, show_default=True, metavar='INT', help='t_init, in [0,999]')),
    (('--fp16',), dict(type=bool, default=False, show_default=True, metavar='BOOL', help='Reference fp16 recipe (optimizer eps 1e-6)')),
    (('--precision',), dict(type=click.Choice(['bf16', 'fp32']), default='bf16', show_default=True, help='Compute dtype of the HIP path (not a reference option)')),
    (('--deterministic',), dict(type=bool, default=False, show_default=True, metavar='BOOL', help='Bit-reproducible training step: order-fixed gradient reductions (not a reference option)')),
    (('--snapshot_images',), dict(type=bool, default=False, show_default=True, metavar='BOOL', help='Write the preview grids fakes_init.png and fakes_<alpha>_<kimg>_{1,2,4}.png at the snapshot ticks; the reference does this whenever --metrics is set (not a reference option)')),
    (('--teacher-weights', 'teacher_weights'), dict(type=click.Choice(['bf16', 'fp8', 'fp8-frozen']), default='bf16', show_default=True, help='fp8: frozen teacher forward weights as e4m3 + per-channel scales; fp8-frozen: every pass without weight gradients (not a reference option)')),
    (('--ls',), dict(type=click.FloatRange(min=0, min_open=True), default=1, show_default=True, help='Loss scaling')),
    (('--lsg',), dict(type=click.FloatRange(min=0, min_open=True), default=1, show_default=True, help='Loss scaling G')),
    (('--alpha',), dict(type=click.FloatRange(min=-1000, min_open=True), default=1, show_default=True, help='L2-alpha*L1')),
    (('--tmax',), dict(type=click.IntRange(min=0), default=980, show_default=True, help='Largest teacher time step')),
    (('--tmin',), dict(type=click.IntRange(min=0), default=20, show_default=True, help='Smallest teacher time step')),
    (('--lr',), dict(type=click.FloatRange(min=0, min_open=True), default=1e-6, show_default=True, help='Fake-score learning rate')),
    (('--glr',), dict(type=click.FloatRange(min=0, min_open=True), default=1e-6, show_default=True, help='Generator learning rate')),
    (('--train_mode',), dict(type=bool, default=True, show_default=True, help='Distill (True) or evaluate the metrics of --network_pkl with 1 / 2 / 4 generation steps (False)')),
    (('--network_pkl',), dict(type=str, default=None, help='network-snapshot-*.pkl to evaluate with --train_mode 0, or "teacher": the teacher of --sd_model itself')),
    (('--teacher_steps',), dict(type=int, default=None, metavar='INT', help=f'DDIM steps of --network_pkl teacher  [default: {TEACHER_STEPS}] (not a reference option)')),
    (('--teacher_cfg',), dict(type=float, default=None, help=f'Guidance scale of --network_pkl teacher  [default: {TEACHER_CFG}] (not a reference option)')),
    (('--text_encoder',), dict(type=click.Choice(['torch', 'hip']), default=None, help='CLIP text encoder: the PyTorch module, or the same weights on the HIP kernels  [default: $SIDLSG_TEXT_ENCODER, else torch] (not a reference option)')),
    (('--teacher_sampler',), dict(type=click.Choice(['ddim', 'dpmpp2m']), default=None, help='Solver of --network_pkl teacher: DDIM or DPM-Solver++ 2M  [default: ddim] (not a reference option)')),
    (('--teacher_spacing',), dict(type=click.Choice(['leading', 'trailing', 'linspace']), default=None, help='Timestep spacing of --network_pkl teacher  [default: the timestep_spacing of --sd_model] (not a reference option)')),
    (('--teacher_eta',), dict(type=click.FloatRange(min=0), default=None, help='DDIM eta of --network_pkl teacher  [default: 0] (not a reference option)')),
    (('--teacher_rescale',), dict(type=click.FloatRange(min=0, max=1), default=None, help='Guidance rescale phi (Lin et al. 2024) of --network_pkl teacher  [default: 0] (not a reference option)')),
    (('--cfg_train_fake',), dict(type=float, default=1, show_default=True, help='kappa1: guidance scale when training the fake score')),
    (('--cfg_eval_fake',), dict(type=float, default=1, show_default=True, help='kappa2 = kappa3: guidance scale when evaluating the fake score')),
    (('--cfg_eval_real',), dict(type=float, default=1, show_default=True, help='kappa4: guidance scale when evaluating the teacher')),
    (('--metric_pt_path',), dict(type=str, default=None, help='Accepted for compatibility')),
    (('--metric_clip_path',), dict(type=str, default=None, help='CLIP model behind clipscore30k: a local directory in the Hugging Face layout (config.json, model.safetensors, vocab.json, merges.txt)')),
    (('--metric_open_clip_path',), dict(type=str, default=None, help='CLIP model behind open_clipscore_30k: such a directory, or a pickled open_clip wrapper of the reference')),
    (('--metric_hps_path',), dict(type=str, default=None, metavar='FILE', help='Scorer behind hpsv2: HPS_v2_compressed.pt, or any checkpoint in open_clip\'s layout (.pt / .bin / .safetensors) (not a reference option)')),
    (('--metric_cmmd_clip_path',), dict(type=str, default=None, metavar='DIR', help='CLIP model behind cmmd30k_full / cmmd_test (ViT-L/14-336 in the published CMMD): a local directory in the Hugging Face layout, or random:clip-<arch> (not a reference option)')),
    (('--metric_lpips_vgg',), dict(type=str, default=None, metavar='SPEC', help="LPIPS-VGG backbone behind lpipsdiv1k_full / lpipsdiv_test: a torch.save'd torchvision VGG16 state dict, or random:lpips-vgg[:seed] (not a reference option)")),
    (('--metric_lpips_lin',), dict(type=str, default=None, metavar='SPEC', help="LPIPS lin weights behind lpipsdiv1k_full / lpipsdiv_test: the lpips package's vgg.pth, or random:lpips-vgg[:seed] (not a reference option)")),
    (('--hps_prompts',), dict(type=str, default=None, metavar='DIR', help='HPSv2 benchmark prompts: a directory with anime.json, concept-art.json, paintings.json, photo.json (not a reference option)')),
    (('--hps_arch',), dict(type=str, default=None, help='open_clip architecture of --metric_hps_path  [default: ViT-H-14] (not a reference option)')),
    (('--hps_tokenizer',), dict(type=str, default=None, metavar='DIR', help='vocab.json / merges.txt of the scorer  [default: <sd_model>/tokenizer] (not a reference option)')),
    (('--enable_xformers',), dict(type=bool, default=True, show_default=True, help='Accepted for compatibility (attention is the fused HIP kernel)')),
    (('--gradient_checkpointing',), dict(type=bool, default=False, show_default=True, help='Accepted for compatibility')),
    (('--optimizer',), dict(type=click.Choice(['adam', 'adamw']), default='adam', show_default=True, help='Optimizer')),
    (('--num_steps',), dict(type=click.IntRange(min=1), default=1, show_default=True, help='Number of generation steps of the trained generator')),
    (('--fake_score_use_lora',), dict(type=bool, default=False, show_default=True, help='Unsupported (must be False)')),
    (('--lora',), dict(type=str, multiple=True, metavar='SPEC', help='LoRA file fused into the UNet and the text encoder of --sd_model before the teacher, the fake score and the generator are copied from it (repeatable): a local kohya / diffusers .safetensors / .bin / .pt file, or random:lora[:rank[:seed]] (not a reference option)')),
    (('--lora_scale',), dict(type=float, multiple=True, help='Scale of --lora (repeatable: one for all files, or one per file; negative allowed)  [default: 1] (not a reference option)')),
]


def _with_options(fn):
    for flags, kw in reversed(OPTIONS):
        fn = click.option(*flags, **kw)(fn)
    return fn


TEACHER_SOLVER_OPTIONS = ('teacher_sampler', 'teacher_spacing', 'teacher_eta', 'teacher_rescale')      # sd_util.teacher_sample_solver


def build_config(o):
    """Options -> training_loop kwargs (the reference's `c`, sid_train.py:196-330)."""
    c = EasyDict()
    if o.metrics is not None:
        # FID / CLIP scores at the snapshot ticks (sid_lsg_amd/metrics.py): the feature detector (--metric_pt_path: the
        # TorchScript Inception the reference downloads) and the real-set statistics (--data_stat: a .npz with mu / sigma, or
        # the reference's cached FeatureStats pickle) must be LOCAL files -- there is no network to fetch them from
        from sid_lsg_amd import metrics as _metrics
        bad = [m for m in o.metrics if not _metrics.is_valid_metric(m)]
        if bad:
            raise click.ClickException(f'--metrics: unknown {bad}; valid: {_metrics.list_valid_metrics()}')
        from sid_lsg_amd.data import has_image_files
        has_images = has_image_files(o.data)
        needs_images = [m for m in o.metrics if m in _metrics.NEEDS_IMAGES]
        # --data_stat may be left out when the statistics can be computed from the images of --data
        hps = [m for m in o.metrics if m in _metrics.HPS_METRICS]      # scored by --metric_hps_path alone: no Inception file, no statistics
        cmmd = [m for m in o.metrics if m in _metrics.CMMD_METRICS]    # scored by --metric_cmmd_clip_path and the real images: likewise
        inception_score = [m for m in o.metrics if m in _metrics.IS_METRICS]      # the detector's class probabilities of the generated images: no statistics
        lpipsdiv = [m for m in o.metrics if m in _metrics.LPIPSDIV_METRICS]      # scored by --metric_lpips_vgg / --metric_lpips_lin alone: no Inception file, no statistics
        need_stat = o.data_stat is not None or (len(needs_images) + len(hps) + len(inception_score) + len(lpipsdiv) < len(o.metrics) and not has_images)
        need_pt = len(hps) + len(cmmd) + len(lpipsdiv) < len(o.metrics)
        for flag, path in ((('--metric_pt_path', o.metric_pt_path),) if need_pt else ()) + ((('--data_stat', o.data_stat),) if need_stat else ()):
            if flag == '--metric_pt_path' and _metrics.is_inception_spec(path):      # random:inception-v3[:seed], built by sid_lsg_amd.inception
                continue
            if not path or not os.path.isfile(path):
                raise click.ClickException(f'--metrics needs {flag} to be a local file (got {path!r})')
        if hps:
            if not o.get('metric_hps_path') or not os.path.isfile(o.metric_hps_path):
                raise click.ClickException(f'--metrics {",".join(hps)} needs --metric_hps_path to be a local file (got {o.get("metric_hps_path")!r})')
            if not o.get('hps_prompts') or not os.path.isdir(o.hps_prompts):
                raise click.ClickException(f'--metrics {",".join(hps)} needs --hps_prompts to be a local directory (got {o.get("hps_prompts")!r})')
        if cmmd and not _metrics.is_clip_spec(o.get('metric_cmmd_clip_path')):
            raise click.ClickException(f'--metrics {",".join(cmmd)} needs --metric_cmmd_clip_path to be a local CLIP directory in the Hugging Face '
                                       f'layout or random:clip-<arch> (got {o.get("metric_cmmd_clip_path")!r})')
        if lpipsdiv:
            from sid_lsg_amd import fidelity as _fidelity
            try:
                _fidelity.check_specs(o.get('metric_lpips_vgg'), o.get('metric_lpips_lin'))
                for flag in ('metric_lpips_vgg', 'metric_lpips_lin'):
                    if not _fidelity.is_random_spec(o[flag]) and not os.path.isfile(o[flag]):
                        raise ValueError(f'--{flag} {o[flag]!r}: not a local file')
            except ValueError as e:
                raise click.ClickException(f'--metrics {",".join(lpipsdiv)}: ' + str(e).replace('--lpips_', '--metric_lpips_'))
        if needs_images and not has_images:
            raise click.ClickException(f'--metrics {",".join(needs_images)} read the real images: --data must be a directory of images '
                                       f'with .txt captions (got {o.data!r})')
    if o.fake_score_use_lora:
        raise click.ClickException('--fake_score_use_lora is not supported')
    if not o.train_mode:
        if o.metrics is None:
            raise click.ClickException('--train_mode 0 evaluates a network snapshot: --metrics is required')
        if o.network_pkl != TEACHER and (not o.network_pkl or not os.path.isfile(o.network_pkl)):
            raise click.ClickException(f'--train_mode 0 needs --network_pkl to be a local network-snapshot-*.pkl (got {o.network_pkl!r})')
    teacher = not o.train_mode and o.network_pkl == TEACHER
    given = [f'--{k}' for k in ('teacher_steps', 'teacher_cfg') + TEACHER_SOLVER_OPTIONS if o.get(k) is not None]
    if given and not teacher:
        raise click.ClickException(f'{" / ".join(given)} apply to --train_mode 0 --network_pkl {TEACHER} only')
    c.metrics, c.resolution = o.metrics, o.resolution
    c.metric_real_stats = o.data_stat
    if o.metrics is not None and o.data:
        # the evaluation caption set (reference: training.mscoco_dataset.ImageDataset on --data, sid_train.py:232-235)
        # with the pixels only where they are read: precision / recall, statistics without --data_stat, reals.png
        images = has_images and bool(needs_images or o.data_stat is None or o.get('snapshot_images', False))
        cls = 'ImageCaptionDataset' if images else 'CaptionDataset'
        c.dataset_kwargs = EasyDict(class_name=f'sid_lsg_amd.data.{cls}', path=o.data, resolution=o.resolution, random_flip=o.xflip)
        # fail at start-up, not at the first metrics tick hours into the run: the set is only constructed there
        try:
            construct_class_by_name(**c.dataset_kwargs)
        except OSError as e:
            raise click.ClickException(f'--metrics with --data {o.data!r}: {e} (an image + .txt caption directory, or a text file with one caption per line)')
    c.data_loader_kwargs = EasyDict(pin_memory=True, num_workers=o.workers, prefetch_factor=2)
    c.dataset_prompt_text_kwargs = EasyDict(class_name='sid_lsg_amd.data.PromptDataset', path=o.data_prompt_text,
                                            resolution=o.resolution, random_flip=o.xflip, prompt_only=True)
    eps = 1e-6 if o.fp16 else 1e-8
    cls = 'torch.optim.Adam' if o.optimizer == 'adam' else 'torch.optim.AdamW'      # mapped to the fused HIP optimizer by the loop
    extra = {} if o.optimizer == 'adam' else dict(weight_decay=0.01)
    c.fake_score_optimizer_kwargs = EasyDict(class_name=cls, lr=o.lr, betas=[0.0, 0.999], eps=eps, **extra)
    c.g_optimizer_kwargs = EasyDict(class_name=cls, lr=o.glr, betas=[0.0, 0.999], eps=eps, **extra)
    c.network_kwargs = EasyDict(use_fp16=o.fp16, compute_dtype=o.get('precision', 'bf16'), teacher_weights=o.get('teacher_weights', 'bf16'))
    c.loss_kwargs = EasyDict()
    c.deterministic = bool(o.get('deterministic', False))
    if o.get('snapshot_images', False):      # (absent when off: the printed options of a run without it stay as they were)
        c.snapshot_images = True
    c.init_timestep = o.init_timestep
    c.total_kimg = max(int(o.duration * 1000), 1)
    c.ema_halflife_kimg = int(o.ema * 1000)
    c.update(batch_size=o.batch, batch_gpu=o.batch_gpu, loss_scaling=o.ls, loss_scaling_G=o.lsg, cudnn_benchmark=o.bench,
             kimg_per_tick=o.tick, snapshot_ticks=o.snap, state_dump_ticks=o.dump, alpha=o.alpha, tmax=o.tmax, tmin=o.tmin)
    c.update(cfg_train_fake=o.cfg_train_fake, cfg_eval_fake=o.cfg_eval_fake, cfg_eval_real=o.cfg_eval_real, num_steps=o.num_steps,
             train_mode=bool(o.train_mode), network_pkl=o.network_pkl, fake_score_use_lora=False, enable_xformers=o.enable_xformers,
             gradient_checkpointing=o.gradient_checkpointing, pretrained_model_name_or_path=o.sd_model,
             pretrained_vae_model_name_or_path=o.sd_model, metric_pt_path=o.metric_pt_path,
             metric_open_clip_path=o.metric_open_clip_path, metric_clip_path=o.metric_clip_path)
    if o.get('text_encoder') is not None:      # (absent when not given: load_sd15 then decides, and the printed options stay as they were)
        c.text_encoder = o.text_encoder
    for k in ('metric_hps_path', 'hps_prompts', 'hps_arch', 'hps_tokenizer', 'metric_cmmd_clip_path', 'metric_lpips_vgg', 'metric_lpips_lin'):      # (absent when not given, likewise)
        if o.get(k) is not None:
            c[k] = o[k]
    if teacher:      # (absent otherwise: the printed options of every other run stay as they were)
        T = resolve_scheduler(o.sd_model).config.num_train_timesteps
        c.teacher_steps = TEACHER_STEPS if o.get('teacher_steps') is None else int(o.teacher_steps)
        c.teacher_cfg = TEACHER_CFG if o.get('teacher_cfg') is None else float(o.teacher_cfg)
        if not 1 <= c.teacher_steps <= T:
            raise click.ClickException(f'--teacher_steps {c.teacher_steps}: expected 1 .. {T} (num_train_timesteps of --sd_model)')
        for k in TEACHER_SOLVER_OPTIONS:      # (absent when not given: the deterministic DDIM path of teacher_sample, as before)
            if o.get(k) is not None:
                c[k] = o[k] if isinstance(o[k], str) else float(o[k])
        if c.get('teacher_sampler') == 'dpmpp2m' and c.get('teacher_eta'):
            raise click.ClickException(f'--teacher_eta {c.teacher_eta:g}: --teacher_sampler dpmpp2m is deterministic (eta applies to ddim)')
        if c.get('teacher_sampler', 'ddim') == 'ddim' and c.get('teacher_spacing') == 'linspace':
            raise click.ClickException('--teacher_spacing linspace: not reproduced for --teacher_sampler ddim (use leading or trailing)')
    if o.get('lora') or o.get('lora_scale'):      # (absent when not given: the printed options of every other run stay as they were)
        from sid_lsg_amd.sd_util import lora_scales
        try:
            c.lora = EasyDict(specs=list(o.get('lora') or ()), scales=lora_scales(len(o.get('lora') or ()), o.get('lora_scale')))
        except ValueError as e:
            raise click.ClickException(str(e))
        for spec in c.lora.specs:
            if not str(spec).lower().startswith('random:') and not os.path.isfile(spec):
                raise click.ClickException(f'--lora {spec}: not a local file (a .safetensors / .bin / .pt LoRA, or random:lora[:rank[:seed]])')
    if o.transfer is not None:
        c.resume_pkl = o.transfer
    if o.resume is not None:
        m = re.fullmatch(r'training-state-(\d+).pt', os.path.basename(o.resume))
        if not m or not os.path.isfile(o.resume):
            raise click.ClickException('--resume must point to training-state-*.pt from a previous training run')
        c.resume_training, c.resume_kimg = o.resume, int(m.group(1))
    return c


def pick_seed(seed):
    if seed is not None:
        return seed
    s = torch.randint(1 << 31, size=[], device=torch.device('cuda'))
    if dist.get_world_size() > 1:
        torch.distributed.broadcast(s, src=0)
    return int(s)


def pick_run_dir(outdir, desc, nosubdir):
    if dist.get_rank() != 0:
        return None
    if nosubdir:
        return outdir
    ids = []
    if os.path.isdir(outdir):
        for x in os.listdir(outdir):
            m = re.match(r'^\d+', x)
            if m and os.path.isdir(os.path.join(outdir, x)):
                ids.append(int(m.group()))
    run_dir = os.path.join(outdir, f'{max(ids, default=-1) + 1:05d}-{desc}')
    assert not os.path.exists(run_dir)
    return run_dir


@click.command()
@_with_options
def main(**kwargs):
    o = EasyDict(kwargs)
    dist.init()
    c = build_config(o)
    try:
        ds = construct_class_by_name(**c.dataset_prompt_text_kwargs)
    except (IOError, OSError) as err:
        raise click.ClickException(f'--data_prompt_text: {err}')
    c.seed = pick_seed(o.seed)
    dtype_str = 'fp16' if o.fp16 else 'fp32'
    desc = (f'{ds.name}-text_cond-glr{o.glr}-lr{o.lr}-initsigma{o.init_timestep}-gpus{dist.get_world_size():d}-alpha{c.alpha}'
            f'-batch{c.batch_size:d}-tmax{c.tmax:d}-{dtype_str}')
    if o.desc is not None:
        desc += f'-{o.desc}'
    c.run_dir = pick_run_dir(o.outdir, desc, o.nosubdir)

    dist.print0()
    dist.print0('Training options:')
    dist.print0(json.dumps(c, indent=2))
    dist.print0()
    dist.print0(f'Output directory:        {c.run_dir}')
    dist.print0(f'Prompts:                 {o.data_prompt_text} ({len(ds)} lines)')
    dist.print0(f'Number of GPUs:          {dist.get_world_size()}')
    dist.print0(f'Batch size:              {c.batch_size}')
    dist.print0(f'Compute:                 bf16 MFMA, fp32 masters (reference recipe: {dtype_str})')
    dist.print0(f'Prediction type:         {resolve_scheduler(o.sd_model).config.prediction_type}')
    dist.print0()
    if o.dry_run:
        dist.print0('Dry run; exiting.')
        return
    if dist.get_rank() == 0:
        os.makedirs(c.run_dir, exist_ok=True)
        with open(os.path.join(c.run_dir, 'training_options.json'), 'wt') as f:
            json.dump(c, f, indent=2)
    training_loop(**c)


if __name__ == '__main__':
    main()
