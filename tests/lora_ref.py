"""Independent fp64 restatement of the LoRA merge, for the tests: its own key walk for both key families, W + scale * alpha / rank *
up @ down per layer in fp64 with the convolution factors contracted by einsum over the rank.  Nothing here imports sid_lsg_amd.lora.

    merge(unet_sd, te_sd, files, scales) -> (merged diffusers-layout UNet state dict, merged transformers-layout text-encoder state dict)

`unet_sd` / `te_sd` are plain state dicts (name -> tensor); the module names a key may address are the `<module>.weight` entries of
these dicts with 2 or 4 dimensions."""
import torch


def _modules(sd):
    return {k[:-len('.weight')]: v for k, v in sd.items() if k.endswith('.weight') and v.dim() in (2, 4)}


def walk(file_sd, unet_sd, te_sd):
    """-> {('unet' | 'te', module): dict(down=, up=, alpha=)} from kohya or diffusers keys."""
    nets = {'unet': _modules(unet_sd), 'te': _modules(te_sd or {})}
    flat = {net: {m.replace('.', '_'): m for m in mods} for net, mods in nets.items()}
    out = {}
    for key, t in file_sd.items():
        if key.startswith('lora_unet_') or key.startswith('lora_te_'):
            net = 'unet' if key.startswith('lora_unet_') else 'te'
            head, tail = key.split('.', 1)
            mod = flat[net][head[len('lora_unet_' if net == 'unet' else 'lora_te_'):]]
            part = {'lora_down.weight': 'down', 'lora_up.weight': 'up', 'alpha': 'alpha'}[tail]
        else:
            net = 'unet' if key.startswith('unet.') else 'te'
            body = key[len('unet.' if net == 'unet' else 'text_encoder.'):]
            for tail, part in (('.lora_A.weight', 'down'), ('.lora_B.weight', 'up'), ('.lora.down.weight', 'down'), ('.lora.up.weight', 'up'),
                               ('.alpha', 'alpha')):
                if body.endswith(tail):
                    mod = body[:-len(tail)]
                    break
            else:
                raise KeyError(key)
            assert mod in nets[net], key
        out.setdefault((net, mod), {})[part] = t
    return out


def delta(w, down, up, alpha):
    """alpha / rank * (up @ down) in fp64, in the shape of w (diffusers layout)."""
    down, up = down.double(), up.double()
    rank = down.shape[0]
    if w.dim() == 4:
        d4 = down if down.dim() == 4 else down[:, :, None, None]
        u2 = up.reshape(up.shape[0], rank)
        d = torch.einsum('or,rikl->oikl', u2, d4)
    else:
        d = torch.einsum('or,ri->oi', up.reshape(up.shape[0], rank), down.reshape(rank, -1))
    assert d.shape == w.shape, (d.shape, w.shape)
    return d * (alpha / rank)


def merge(unet_sd, te_sd, files, scales):
    """fp64 merged copies of both state dicts (every tensor converted to fp64; only the addressed weights change)."""
    out = {'unet': {k: v.detach().double().cpu().clone() for k, v in unet_sd.items()},
           'te': {k: v.detach().double().cpu().clone() for k, v in (te_sd or {}).items()}}
    for file_sd, scale in zip(files, scales):
        for (net, mod), parts in walk(file_sd, unet_sd, te_sd).items():
            rank = parts['down'].shape[0]
            alpha = float(parts['alpha']) if 'alpha' in parts else float(rank)
            w = out[net][mod + '.weight']
            w += float(scale) * delta(w, parts['down'].cpu(), parts['up'].cpu(), alpha)
    return out['unet'], out['te']


def kohya_to_diffusers(file_sd, unet_sd, te_sd, style='peft'):
    """The same factors under diffusers / PEFT keys (`style` 'peft': lora_A / lora_B, 'old': lora.down / lora.up)."""
    names = {'peft': ('lora_A.weight', 'lora_B.weight'), 'old': ('lora.down.weight', 'lora.up.weight')}[style]
    out = {}
    for (net, mod), parts in walk(file_sd, unet_sd, te_sd).items():
        head = ('unet.' if net == 'unet' else 'text_encoder.') + mod
        out[f'{head}.{names[0]}'] = parts['down']
        out[f'{head}.{names[1]}'] = parts['up']
        if 'alpha' in parts:
            out[f'{head}.alpha'] = parts['alpha']
    return out
