"""Build libsidlsg_hip.so (gfx950) in-tree with plain hipcc.  `python -m sid_lsg_amd.csrc.build`."""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
SOURCES = ['gemm.hip', 'gemm_fp8.hip', 'wgrad.hip', 'state.hip', 'norm.hip', 'attention.hip', 'elementwise.hip', 'optim.hip', 'fp32.hip', 'trace.hip', 'image_grid.hip', 'pr_dist.hip', 'clip.hip', 'attn_wide.hip', 'vae_io.hip', 'text.hip', 'hps.hip', 'solver.hip', 'inpaint.hip', 'mmd.hip', 'inception.hip', 'controlnet.hip', 'ip_attn.hip', 'fidelity.hip', 'lora.hip', 'canny.hip']
LIB = os.path.join(PKG, 'libsidlsg_hip.so')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-munsafe-fp-atomics', '-Wno-unused-result']
# Per-file extras.  attention.hip: the softmax works on MFMA results with VALU ops; with the default heuristics the
# accumulators live in AGPRs and every tile pays ~110 v_accvgpr_read/write moves in a VALU-bound loop.
# -fno-honor-nans: no canonicalising v_max x,x in front of every fmaxf on an MFMA result (infinities stay honoured).
# image_grid.hip: the preview grid's uint8 conversion is specified rounding by rounding (subtract, multiply, round to even).
# clip.hip: likewise the CLIP preprocessing (divide, bicubic taps, normalise): its result must not depend on compiler fusion.
# vae_io.hip: likewise the VAE encoder's image conversion (divide, subtract) and its posterior tail (mean + std * eps).
# hps.hip: likewise the float tail of the HPSv2 preprocessing (divide, subtract, divide).
# inpaint.hip: likewise the known region of the masked step boundary (a rounded product, then one fma), bit-equal to noisy_input's x_t.
# controlnet.hip: likewise the control image's conversion (one division).
# inception.hip: likewise the detector's input resize (two lerps, subtract, divide); its MFMA contractions are not affected.
# fidelity.hip: likewise the SSIM moments and formula (fp64), the LPIPS input (divide, subtract, subtract, divide) and the per-tap distance.
EXTRA = {'attention.hip': ['-mllvm', '-amdgpu-mfma-vgpr-form', '-fno-honor-nans'], 'image_grid.hip': ['-ffp-contract=off'],
         'clip.hip': ['-ffp-contract=off'], 'vae_io.hip': ['-ffp-contract=off'], 'hps.hip': ['-ffp-contract=off'], 'inpaint.hip': ['-ffp-contract=off'],
         'inception.hip': ['-ffp-contract=off'], 'controlnet.hip': ['-ffp-contract=off'], 'fidelity.hip': ['-ffp-contract=off']}


def digest():
    h = hashlib.md5()
    for f in SOURCES + sorted(f for f in os.listdir(HERE) if f.endswith('.h')):      # every header: a new one cannot leave a stale library
        with open(os.path.join(HERE, f), 'rb') as fh:
            h.update(fh.read())
    with open(os.path.join(os.path.dirname(PKG), 'include', 'sidlsg_hip.h'), 'rb') as fh:      # gemm_core.h includes the C ABI header
        h.update(fh.read())
    h.update((' '.join(FLAGS) + repr(sorted(EXTRA.items()))).encode())
    return h.hexdigest()


def build(force=False, verbose=True):
    stamp = LIB + '.md5'
    d = digest()
    if not force and os.path.isfile(LIB) and os.path.isfile(stamp) and open(stamp).read().strip() == d:
        return LIB
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, 'build'), exist_ok=True)
    for src in SOURCES:
        obj = os.path.join(HERE, 'build', src.replace('.hip', '.o'))
        objs.append(obj)
        cmd = [hipcc] + FLAGS + EXTRA.get(src, []) + ['-c', os.path.join(HERE, src), '-o', obj]
        if verbose:
            print(' '.join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f'hipcc failed on {src}')
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC'] + objs + ['-o', LIB]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(stamp, 'w') as f:
        f.write(d)
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv))
