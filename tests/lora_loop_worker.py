"""Child process of tests/test_gpu_lora.py::test_sid_train_with_a_lora: the training loop on random:tiny for two iterations, three times --
without `lora`, with an empty LoRA list, with random:lora -- in deterministic mode.  Saves per run the losses, the generator's masters and
the path of the last snapshot.

    python tests/lora_loop_worker.py OUT.pt WORK_DIR"""
import glob
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RESOLUTION, BATCH, ITERATIONS, LR = 64, 4, 2, 1e-6


def loop_kwargs(run_dir, prompt_dir, device, **extra):
    from sid_lsg_amd.dnnlib_util import EasyDict
    kw = dict(run_dir=str(run_dir), network_kwargs=EasyDict(use_fp16=False),
              dataset_prompt_text_kwargs=EasyDict(class_name='sid_lsg_amd.data.PromptDataset', path=str(prompt_dir), resolution=RESOLUTION,
                                                  prompt_only=True),
              fake_score_optimizer_kwargs=EasyDict(class_name='torch.optim.Adam', lr=LR, betas=[0.0, 0.999], eps=1e-8),
              g_optimizer_kwargs=EasyDict(class_name='torch.optim.Adam', lr=LR, betas=[0.0, 0.999], eps=1e-8),
              seed=1, batch_size=BATCH, batch_gpu=BATCH, total_kimg=ITERATIONS * BATCH / 1000.0, ema_halflife_kimg=0.008, ema_rampup_ratio=None,
              kimg_per_tick=BATCH / 1000.0, snapshot_ticks=1, state_dump_ticks=None, alpha=1.0, tmax=980, tmin=20, device=device, metrics=None,
              init_timestep=625, pretrained_model_name_or_path='random:tiny', cfg_train_fake=1.5, cfg_eval_fake=1.5, cfg_eval_real=1.5,
              resolution=RESOLUTION, deterministic=True)
    kw.update(extra)
    return kw


if __name__ == '__main__':
    out, work = sys.argv[1], sys.argv[2]
    from sid_lsg_amd.dnnlib_util import EasyDict
    from sid_lsg_amd.training_loop import training_loop
    prompt_dir = os.path.join(work, 'prompts')
    os.makedirs(prompt_dir, exist_ok=True)
    with open(os.path.join(prompt_dir, 'aesthetics_6_plus.txt'), 'w') as f:
        f.write('\n'.join(f'a photo of object number {i}' for i in range(40)) + '\n')
    result = dict(lr=LR)
    for tag, extra in (('none', {}), ('empty', dict(lora=EasyDict(specs=[], scales=[]))), ('lora', dict(lora=EasyDict(specs=['random:lora'], scales=[1.0])))):
        run_dir = os.path.join(work, 'run_' + tag)
        os.makedirs(run_dir, exist_ok=True)
        losses = []
        nets = training_loop(on_iteration=lambda it, lf, lg: losses.extend([lf, lg]), **loop_kwargs(run_dir, prompt_dir, torch.device('cuda'), **extra))
        torch.cuda.synchronize()
        result[tag] = dict(losses=torch.tensor(losses, dtype=torch.float64), G=nets['G'].flat_params.detach().cpu(),
                           snapshot=sorted(glob.glob(os.path.join(run_dir, 'network-snapshot-*.pkl')))[-1])
    torch.save(result, out)
