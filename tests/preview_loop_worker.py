"""Child process of tests/test_gpu_preview.py: the tiny product loop, one iteration per tick and a snapshot at every tick, with the
preview grids on or off.
    python tests/preview_loop_worker.py OUT.pt RUN_DIR PROMPT_DIR {0|1}
saves the per-iteration losses (through on_iteration) and the final G / G_ema parameters; the caller sets SIDLSG_DETERMINISTIC."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RESOLUTION, BATCH, ITERATIONS = 512, 4, 3


def loop_kwargs(run_dir, prompt_dir, device, **extra):
    from sid_lsg_amd.dnnlib_util import EasyDict
    kw = dict(run_dir=str(run_dir), network_kwargs=EasyDict(use_fp16=False),
              dataset_prompt_text_kwargs=EasyDict(class_name='sid_lsg_amd.data.PromptDataset', path=str(prompt_dir), resolution=RESOLUTION,
                                                  prompt_only=True),
              fake_score_optimizer_kwargs=EasyDict(class_name='torch.optim.Adam', lr=1e-4, betas=[0.0, 0.999], eps=1e-8),
              g_optimizer_kwargs=EasyDict(class_name='torch.optim.Adam', lr=1e-4, betas=[0.0, 0.999], eps=1e-8),
              seed=1, batch_size=BATCH, batch_gpu=BATCH, total_kimg=ITERATIONS * BATCH / 1000.0, ema_halflife_kimg=0.008, ema_rampup_ratio=None,
              kimg_per_tick=BATCH / 1000.0, snapshot_ticks=1, state_dump_ticks=None, alpha=1.0, tmax=980, tmin=20, device=device, metrics=None,
              init_timestep=625, pretrained_model_name_or_path='random:tiny', cfg_train_fake=1.5, cfg_eval_fake=1.5, cfg_eval_real=1.5,
              resolution=RESOLUTION)
    kw.update(extra)
    return kw


def write_prompts(prompt_dir):
    os.makedirs(prompt_dir, exist_ok=True)
    with open(os.path.join(prompt_dir, 'aesthetics_6_plus.txt'), 'w') as f:
        f.write('\n'.join(f'a photo of object number {i}' for i in range(40)) + '\n')


if __name__ == '__main__':
    out, run_dir, prompt_dir, on = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4] == '1'
    from sid_lsg_amd.training_loop import training_loop
    os.makedirs(run_dir, exist_ok=True)
    losses = []
    nets = training_loop(on_iteration=lambda it, lf, lg: losses.extend([lf, lg]),
                         **loop_kwargs(run_dir, prompt_dir, torch.device('cuda'), snapshot_images=on))
    torch.cuda.synchronize()
    torch.save(dict(losses=torch.tensor(losses, dtype=torch.float64), G=nets['G'].flat_params.detach().cpu(),
                    G_ema=nets['G_ema'].flat_params.detach().cpu()), out)
