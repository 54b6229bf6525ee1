"""LoRA files (Hu et al. 2021) for the UNet and the text encoder: low-rank updates MERGED into the fp32 master weights, one HIP launch
per network (ops.lora_merge, csrc/lora.hip), followed by the network's own refresh of everything derived from the masters.

    W' = W + sum_i scale_i * alpha_i / rank_i * up_i @ down_i

Two key families are read (`parse_lora`): kohya / A1111 (`lora_unet_<module, '.' -> '_'>.lora_down.weight | .lora_up.weight | .alpha`,
`lora_te_...`) and diffusers / PEFT (`unet.<module>.lora_A.weight | .lora_B.weight` or `.lora.down.weight | .lora.up.weight`,
`text_encoder.<module>...`).  The module part of a key is looked up in a table built from `named_modules()` of the two networks; a key
that is not in the table is refused, never split at a guessed underscore.  The key rules of both families restate kohya's and
diffusers' published loaders: neither package is installed here, so agreement with them is not pinned by a test
(tests/lora_ref.py is an independent fp64 restatement of the same rules).

Why the masters: every compute copy (bf16 forward copies, backward-data operands, pre-scaled q rows, e4m3 copies) is derived from them
by `refresh_compute_weights`, and in the fp32 mode the compute copy IS the master.  The UNet pass itself does not change: a network
with a LoRA attached issues exactly the launches of the plain network.  The price of the attached form is a saved copy of the touched
master ranges (`LoraSet`), from which `set_scales` re-merges and `detach` restores bit for bit; `fuse` keeps nothing.

A network that is pickled, deep-copied or `state_dict()`ed while a LoraSet is attached holds the MERGED weights.
"""
import os
import re

import torch

from . import ops

RANDOM_PREFIX = 'random:lora'
MAX_RANK = ops.LORA_MAX_RANK
F32 = torch.float32

_KOHYA_SUFFIX = {'lora_down.weight': 'down', 'lora_up.weight': 'up', 'alpha': 'alpha'}
_DIFFUSERS_SUFFIX = {'lora_A.weight': 'down', 'lora_B.weight': 'up', 'lora.down.weight': 'down', 'lora.up.weight': 'up', 'alpha': 'alpha'}
_OTHER_ALGO = re.compile(r'(^|[._])(hada_\w+|lokr_\w+)|(^|\.)(dora_scale|lora_magnitude_vector|lora_mid(\.weight)?|diff|diff_b)$')
_SDXL_KOHYA = ('lora_te1_', 'lora_te2_', 'lora_unet_input_blocks_', 'lora_unet_middle_block_', 'lora_unet_output_blocks_', 'lora_unet_out_',
               'lora_unet_time_embed_', 'lora_unet_label_emb_')
_SDXL_DIFFUSERS = ('text_encoder_2.',)


# ------------------------------------------------------------------------------------------------
# files and keys
def read_lora_file(path):
    """A local `.safetensors`, or `.bin` / `.pt` through torch.load(weights_only=True) -> flat dict key -> tensor."""
    name = str(path)
    if not os.path.isfile(name):
        raise FileNotFoundError(f"{name}: not a local LoRA file; pass a .safetensors / .bin / .pt file or '{RANDOM_PREFIX}[:rank[:seed]]'")
    low = name.lower()
    if low.endswith('.safetensors'):
        from safetensors.torch import load_file
        sd = load_file(name)
    elif low.endswith(('.bin', '.pt')):
        sd = torch.load(name, map_location='cpu', weights_only=True)
    else:
        raise ValueError(f'{name}: expected a .safetensors, .bin or .pt file')
    if not isinstance(sd, dict) or not all(isinstance(k, str) and torch.is_tensor(v) for k, v in sd.items()):
        raise ValueError(f'{name}: expected a flat dict of tensors')
    return dict(sd)


def parse_random_spec(spec):
    """'random:lora[:rank[:seed]]' -> (rank, seed or None)."""
    parts = str(spec).lower().split(':')
    if parts[:2] != RANDOM_PREFIX.split(':') or len(parts) > 4 or not all(p.isdigit() for p in parts[2:]):
        raise ValueError(f"{spec}: expected '{RANDOM_PREFIX}[:rank[:seed]]' with non-negative integers")
    rank = int(parts[2]) if len(parts) > 2 else 4
    if rank < 1:
        raise ValueError(f'{spec}: the rank must be at least 1')
    return rank, (int(parts[3]) if len(parts) > 3 else None)


class Layer:
    """One weight a LoRA may address: net 'unet' | 'te', the module name, kind 'linear' | 'conv1x1' | 'conv3x3', and the physical master
    matrix [n][kk] (kk = Cin, or 9 Cin in [3][3][Cin] order for a 3 x 3 convolution)."""

    def __init__(self, net, name, kind, n, cin):
        self.net, self.name, self.kind, self.n, self.cin = net, name, kind, int(n), int(cin)
        self.kk = self.cin * (9 if kind == 'conv3x3' else 1)

    def __repr__(self):
        return f'{self.net}:{self.name}'


def layer_table(unet, text_encoder=None):
    """{(net, module name): Layer} over every target: the HLinear / HConv1x1 / HConv3x3 weights of the UNet and the nn.Linear layers
    of the text encoder."""
    from .unet import HConv3x3, HLinear
    table = {}
    if unet is not None:
        for name, mod in unet.named_modules():
            if isinstance(mod, HConv3x3):
                table[('unet', name)] = Layer('unet', name, 'conv3x3', mod.weight.shape[0], mod.weight.shape[1])
            elif isinstance(mod, HLinear):
                table[('unet', name)] = Layer('unet', name, mod.kind, mod.weight.shape[0], mod.weight.shape[1])
    if text_encoder is not None:
        for name, mod in text_encoder.named_modules():
            if isinstance(mod, torch.nn.Linear):
                table[('te', name)] = Layer('te', name, 'linear', mod.weight.shape[0], mod.weight.shape[1])
    return table


def _name_tables(table):
    """kohya's flattened names and diffusers' dotted ones -> (net, module).  Two modules that flatten to one name would make a key
    ambiguous: that is an error here, not a guess."""
    kohya, dotted = {}, {}
    for (net, name) in table:
        k = ('lora_unet_' if net == 'unet' else 'lora_te_') + name.replace('.', '_')
        if k in kohya:
            raise RuntimeError(f'modules {kohya[k][1]} and {name} share the kohya name {k}')
        kohya[k] = (net, name)
        dotted[('unet.' if net == 'unet' else 'text_encoder.') + name] = (net, name)
    return kohya, dotted


def _refuse_family(key):
    if _OTHER_ALGO.search(key):
        raise ValueError(f'{key}: LoHa / LoKr / DoRA / Tucker and full-difference keys are not supported (plain LoRA up / down factors only)')
    if key.startswith(_SDXL_KOHYA) or key.startswith(_SDXL_DIFFUSERS):
        raise ValueError(f'{key}: an SDXL / LDM-layout LoRA key; only SD 1.x / 2.x files with diffusers module names are supported')


def parse_lora(sd, unet, text_encoder=None, where='LoRA state'):
    """Flat state dict -> [(target, down, up, alpha, rank)], target = ('unet' | 'te', module name), down / up CPU fp32 in the file's own
    shapes (down [r, Cin] or [r, Cin, kh, kw]; up [Cout, r] or [Cout, r, 1, 1]), alpha a float (the rank when the file has none), in the
    order of the networks' modules.  Everything the module docstring lists as refused raises a ValueError naming the key."""
    table = layer_table(unet, text_encoder)
    kohya, dotted = _name_tables(table)
    found = {}        # target -> {'down': (key, t), 'up': ..., 'alpha': ...}
    for key, t in sd.items():
        _refuse_family(key)
        target = part = None
        if key.startswith('lora_'):
            head, _, tail = key.partition('.')
            part = _KOHYA_SUFFIX.get(tail)
            if part is None:
                raise ValueError(f'{where}: {key}: not a LoRA key (expected .lora_down.weight, .lora_up.weight or .alpha)')
            target = kohya.get(head)
        elif key.startswith(('unet.', 'text_encoder.')):
            for suffix, p in _DIFFUSERS_SUFFIX.items():
                if key.endswith('.' + suffix):
                    part, target = p, dotted.get(key[:-len(suffix) - 1])
                    break
            if part is None:
                raise ValueError(f'{where}: {key}: not a LoRA key (expected .lora_A.weight / .lora_B.weight, .lora.down.weight / .lora.up.weight or .alpha)')
        else:
            raise ValueError(f'{where}: {key}: not a LoRA key (expected a lora_unet_ / lora_te_ or unet. / text_encoder. prefix)')
        if target is None:
            raise ValueError(f'{where}: {key}: no such module in the ' + ('text encoder' if key.startswith(('lora_te', 'text_encoder')) else 'UNet')
                             + ' (the name is looked up whole, underscores are not split by guessing)')
        slot = found.setdefault(target, {})
        if part in slot:
            raise ValueError(f'{where}: {key}: {slot[part][0]} already gives the {part} of {target[1]}')
        slot[part] = (key, t)
    if not found:
        raise ValueError(f'{where}: no LoRA key at all')
    out = []
    for target, layer in table.items():
        slot = found.get(target)
        if slot is None:
            continue
        if 'down' not in slot or 'up' not in slot:
            have = slot.get('down') or slot.get('up') or slot.get('alpha')
            raise ValueError(f'{where}: {have[0]}: ' + ('an up factor without its down' if 'up' in slot else 'a down factor without its up' if 'down' in slot
                                                         else 'an alpha without factors'))
        (kd, down), (ku, up) = slot['down'], slot['up']
        down, up = down.detach().to('cpu', F32), up.detach().to('cpu', F32)
        rank = down.shape[0] if down.dim() else 0
        if rank == 0 or down.numel() == 0 or up.numel() == 0:
            raise ValueError(f'{where}: {kd}: rank 0')
        ksz = 3 if layer.kind == 'conv3x3' else 1
        ok_down = [(rank, layer.cin, ksz, ksz)] + ([(rank, layer.cin)] if ksz == 1 else [])
        if tuple(down.shape) not in ok_down:
            raise ValueError(f'{where}: {kd} has shape {tuple(down.shape)}: {layer.kind} layer {layer.name} takes {" or ".join(map(str, ok_down))}')
        ok_up = [(layer.n, rank, 1, 1)] + ([(layer.n, rank)] if ksz == 1 else [])
        if tuple(up.shape) not in ok_up:
            raise ValueError(f'{where}: {ku} has shape {tuple(up.shape)}: {layer.kind} layer {layer.name} takes {" or ".join(map(str, ok_up))}')
        alpha = float(rank)
        if 'alpha' in slot:
            ka, a = slot['alpha']
            if a.numel() != 1:
                raise ValueError(f'{where}: {ka} has shape {tuple(a.shape)}: expected one number')
            alpha = float(a.detach().float().reshape(()))
        out.append((target, down, up, alpha, rank))
    return out


def physical_down(down, kind):
    """The file's down factor -> [r][kk] in the master's physical column order: [r, Cin] as is, [r, Cin, 3, 3] -> [r][3][3][Cin]."""
    if kind == 'conv3x3':
        return down.permute(0, 2, 3, 1).reshape(down.shape[0], -1).contiguous()
    return down.reshape(down.shape[0], -1).contiguous()


def physical_up(up):
    return up.reshape(up.shape[0], -1).contiguous()


def random_lora_state_dict(unet, text_encoder=None, rank=4, seed=0, unet_state=None):
    """Seeded kohya-keyed LoRA over EVERY target of both networks, both factors non-zero (a real LoRA starts with up = 0, which would
    make every test of the merge vacuous).  alpha = rank; the factors are N(0, s^2) with s^4 = 0.09 |W|_F^2 / (rank n kk), which puts
    |up @ down|_F at about 0.3 |W|_F for every layer.  `unet_state`: the UNet's weights as a diffusers-layout state dict, for a UNet
    that is not materialised (host tests)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    masters = _master_views(unet, text_encoder)
    for (net, name), layer in layer_table(unet, text_encoder).items():
        w = masters[(net, name)]
        if net == 'unet' and unet_state is not None:
            w = unet_state[name + '.weight']
        if w.is_meta:
            raise RuntimeError(f'{layer}: the UNet is not materialised: pass unet_state')
        w = w.detach().float().cpu()
        s = (0.09 * float(w.pow(2).sum()) / (rank * layer.n * layer.kk)) ** 0.25
        head = ('lora_unet_' if net == 'unet' else 'lora_te_') + name.replace('.', '_')
        ksz = 3 if layer.kind == 'conv3x3' else 1
        dshape = (rank, layer.cin, ksz, ksz) if layer.kind != 'linear' else (rank, layer.cin)
        ushape = (layer.n, rank, 1, 1) if layer.kind != 'linear' else (layer.n, rank)
        sd[head + '.lora_down.weight'] = torch.randn(dshape, generator=g) * s
        sd[head + '.lora_up.weight'] = torch.randn(ushape, generator=g) * s
        sd[head + '.alpha'] = torch.tensor(float(rank))
    return sd


def _master_views(unet, text_encoder):
    """{(net, module name): the weight parameter} of every target."""
    out = {}
    mods = {'unet': dict(unet.named_modules()) if unet is not None else {}, 'te': dict(text_encoder.named_modules()) if text_encoder is not None else {}}
    for (net, name) in layer_table(unet, text_encoder):
        out[(net, name)] = mods[net][name].weight
    return out


# ------------------------------------------------------------------------------------------------
# host plan: which columns of which layer belong to which file
class HostPlan:
    """The host side of one network's merge: per touched layer the concatenated, zero-padded factors in two flat CPU buffers and the
    column ranges of the files.

      layers: [dict(layer=Layer, r=columns used, rp=r padded to a multiple of 4, up_off, down_off, coef_off,
                    cols=[(file index, first column, end column, alpha / rank)])]   in module order
      up [sum n * rp], down [sum rp * kk] (physical column order), ncoef = sum rp;  offsets in elements, all multiples of 4."""

    def __init__(self, net, table, adapters):
        self.net = net
        per = {}
        for fi, entries in enumerate(adapters):
            for target, down, up, alpha, rank in entries:
                if target[0] == net:
                    per.setdefault(target, []).append((fi, down, up, alpha, rank))
        self.layers = []
        ups, downs = [], []
        uo = do = co = 0
        for target, layer in table.items():
            if target not in per:
                continue
            r = sum(e[4] for e in per[target])
            if r > MAX_RANK:
                raise ValueError(f'{layer}: concatenated rank {r} over {len(per[target])} adapter(s) exceeds {MAX_RANK}')
            rp = (r + 3) // 4 * 4
            U, D = torch.zeros(layer.n, rp), torch.zeros(rp, layer.kk)
            cols, c = [], 0
            for fi, down, up, alpha, rank in per[target]:
                U[:, c:c + rank] = physical_up(up)
                D[c:c + rank] = physical_down(down, layer.kind)
                cols.append((fi, c, c + rank, alpha / rank))
                c += rank
            self.layers.append(dict(layer=layer, r=r, rp=rp, up_off=uo, down_off=do, coef_off=co, cols=cols))
            ups.append(U.reshape(-1))
            downs.append(D.reshape(-1))
            uo, do, co = uo + U.numel(), do + D.numel(), co + rp
        self.up = torch.cat(ups) if ups else torch.zeros(0)
        self.down = torch.cat(downs) if downs else torch.zeros(0)
        self.ncoef = co

    def coef(self, scales):
        """The coefficient vector [ncoef] fp32 for per-file scales: scale_i * alpha / rank on a file's columns (rounded to fp32 once, from
        the double product), 0 on the padding."""
        v = torch.zeros(self.ncoef, dtype=torch.float64)
        for L in self.layers:
            for fi, lo, hi, ar in L['cols']:
                v[L['coef_off'] + lo:L['coef_off'] + hi] = float(scales[fi]) * ar
        return v.to(F32)

    def job_table(self, base_ptrs, dst_ptrs, up_ptr, down_ptr, coef_ptr, device):
        """ops.LoraJobTable over this plan: base_ptrs / dst_ptrs are per-layer device addresses, the other three the flat buffers'."""
        recs = [(b, d, up_ptr + 4 * L['up_off'], down_ptr + 4 * L['down_off'], coef_ptr + 4 * L['coef_off'], L['layer'].n, L['layer'].kk, L['rp'])
                for L, b, d in zip(self.layers, base_ptrs, dst_ptrs)]
        return ops.LoraJobTable(recs, device)

    @property
    def names(self):
        return [repr(L['layer']) for L in self.layers]


def check_scales(scales, nfiles):
    scales = [float(s) for s in scales]
    if len(scales) != nfiles:
        raise ValueError(f'{len(scales)} scale(s) for {nfiles} LoRA file(s): one per file')
    for s in scales:
        if s != s or s in (float('inf'), float('-inf')):
            raise ValueError(f'LoRA scale {s}: expected a finite value')
    return scales


# ------------------------------------------------------------------------------------------------
# device side
def _unet_of(unet):
    from .controlnet import HipControlNet
    from .unet import HipUNet2DCondition
    if isinstance(unet, HipControlNet):
        raise TypeError('a LoRA addresses the UNet: a HipControlNet cannot take one')
    if not isinstance(unet, HipUNet2DCondition):
        raise TypeError(f'expected a HipUNet2DCondition, got {type(unet).__name__}')
    if unet._flat is None or unet._flat['p'].device.type != 'cuda':
        raise RuntimeError('the LoRA merge runs on the GPU only (no CPU fallback): materialize the UNet on the device first')
    return unet


def _check_idle():
    if ops._dual is not None:
        raise RuntimeError('a LoRA merge inside a grouped pass (forward_pair / ops.dual_networks): merge before or after it')
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError('a LoRA merge while a graph is being captured: the merge and the refresh are not part of a captured step')


class _NetMerge:
    """One network's device state: factors, coefficients, job table; `base` None = in place."""

    def __init__(self, plan, weights, device, save_base):
        self.plan, self.weights = plan, weights           # weights: per layer the contiguous fp32 [n][kk] device tensor (a master view)
        for L, w in zip(plan.layers, weights):
            if w.dtype != F32 or not w.is_contiguous() or w.device.type != 'cuda' or w.numel() != L['layer'].n * L['layer'].kk:
                raise ValueError(f'{L["layer"]}: the master weight must be a contiguous fp32 device tensor (got {w.dtype}, {tuple(w.shape)})')
        self.up, self.down = plan.up.to(device), plan.down.to(device)
        self.coef = torch.zeros(max(plan.ncoef, 4), device=device, dtype=F32)
        self.base = None
        if save_base:
            offs, o = [], 0
            for w in weights:
                offs.append(o)
                o += w.numel()                          # n * kk is a multiple of 4: every saved range stays 16-byte aligned
            self.base = torch.empty(max(o, 4), device=device, dtype=F32)
            self.base_views = [self.base[b:b + w.numel()] for b, w in zip(offs, weights)]
            for v, w in zip(self.base_views, weights):
                v.copy_(w.reshape(-1))
            base_ptrs = [v.data_ptr() for v in self.base_views]
        else:
            base_ptrs = [w.data_ptr() for w in weights]
        self.table = plan.job_table(base_ptrs, [w.data_ptr() for w in weights], self.up.data_ptr(), self.down.data_ptr(), self.coef.data_ptr(), device)

    def merge(self, scales):
        if not self.plan.layers:
            return
        self.coef[:self.plan.ncoef].copy_(self.plan.coef(scales))
        ops.lora_merge(self.table, self.plan.names)

    def restore(self):
        for v, w in zip(self.base_views, self.weights):
            w.reshape(-1).copy_(v)


def _unet_weights(unet, plan):
    fl = unet._flat
    out = []
    for L in plan.layers:
        layer = L['layer']
        o = fl['offs'][layer.name + '.weight']
        out.append(fl['p'][o:o + layer.n * layer.kk].view(layer.n, layer.kk))
    return out


def _te_weights(text_encoder, plan):
    mods = dict(text_encoder.named_modules())
    out = []
    for L in plan.layers:
        w = mods[L['layer'].name].weight
        if w.dtype != F32:
            raise ValueError(f'{L["layer"]}: text-encoder parameters are {w.dtype}: a LoRA merges into fp32 masters')
        out.append(w.data)
    return out


def _refresh(unet, text_encoder, nets):
    if 'unet' in nets:
        unet.refresh_compute_weights()
    if 'te' in nets and text_encoder is not None and hasattr(text_encoder, '_hip_cache'):
        text_encoder._hip_cache = None


def _plans(unet, text_encoder, adapters):
    table = layer_table(unet, text_encoder)
    if text_encoder is None and any(t[0] == 'te' for entries in adapters for t, *_ in entries):
        raise ValueError('the LoRA has text-encoder layers but no text encoder was given')
    for entries in adapters:
        for target, *_ in entries:
            if target not in table:
                raise ValueError(f'LoRA target {target[0]}:{target[1]} is not a layer of the given networks')
    plans = {'unet': HostPlan('unet', table, adapters)}
    if text_encoder is not None:
        plans['te'] = HostPlan('te', table, adapters)
    return plans


def summary(adapters):
    """Per file: (targets in the UNet, targets in the text encoder, smallest rank, largest rank)."""
    rows = []
    for entries in adapters:
        ranks = [e[4] for e in entries] or [0]
        rows.append((sum(e[0][0] == 'unet' for e in entries), sum(e[0][0] == 'te' for e in entries), min(ranks), max(ranks)))
    return rows


class LoraSet:
    """LoRA adapters ATTACHED to a frozen UNet (and its text encoder): `attach(adapters, scales)` saves the touched master ranges,
    uploads the factors once and merges with one launch per network; `set_scales` rewrites the coefficient vector and repeats launch
    and refresh; `detach` copies the saved ranges back.  After `detach`, and after `set_scales` of all zeros, the masters and the bf16
    forward copies equal those before `attach` under torch.equal.  `detach` restores the bits; a zero scale goes through the launch
    (base + 0), which turns a master of -0.0 into +0.0 (equal, not bit-identical) and needs finite factors (0 * inf is NaN).  `adapters`: one parse_lora result per file.

    While attached the networks HOLD the merged weights: pickling, deepcopy and state_dict() give the adapted model.
    Refused: a network with requires_grad parameters (use `fuse` for training), a HipControlNet, an e4m3-weight UNet
    (enable_fp8_weights; the combination is not tried here), a grouped pass or graph capture in flight, attaching twice."""

    def __init__(self, unet, text_encoder=None):
        self.unet, self.text_encoder = _unet_of(unet), text_encoder
        self._nets = None

    @property
    def attached(self):
        return self._nets is not None

    def _check(self):
        _check_idle()
        if self.unet._train_params or any(p.requires_grad for p in self.unet.parameters()):
            raise RuntimeError('LoraSet.attach on a UNet with requires_grad parameters: an optimizer step would train the merged weights and '
                               'detach would undo it; use lora.fuse for a network that trains')
        if self.text_encoder is not None and any(p.requires_grad for p in self.text_encoder.parameters()):
            raise RuntimeError('LoraSet.attach on a text encoder with requires_grad parameters')
        if 'fp8' in self.unet._flat:
            raise RuntimeError('LoraSet.attach on an e4m3-weight UNet (enable_fp8_weights): not supported')

    @torch.no_grad()
    def attach(self, adapters, scales):
        if self.attached:
            raise RuntimeError('LoraSet.attach: already attached; detach() first (or set_scales to change the scales)')
        self._check()
        scales = check_scales(scales, len(adapters))
        plans = _plans(self.unet, self.text_encoder, adapters)
        dev = self.unet._flat['p'].device
        nets = {'unet': _NetMerge(plans['unet'], _unet_weights(self.unet, plans['unet']), dev, True)}
        if 'te' in plans and plans['te'].layers:
            nets['te'] = _NetMerge(plans['te'], _te_weights(self.text_encoder, plans['te']), dev, True)
        self._nets, self.nfiles, self.scales = nets, len(adapters), scales
        self._launch()
        return self

    def _launch(self):
        for nm in self._nets.values():
            nm.merge(self.scales)
        _refresh(self.unet, self.text_encoder, self._nets)

    @torch.no_grad()
    def set_scales(self, scales):
        if not self.attached:
            raise RuntimeError('LoraSet.set_scales: nothing attached')
        _check_idle()
        self.scales = check_scales(scales, self.nfiles)
        self._launch()

    @torch.no_grad()
    def detach(self):
        if not self.attached:
            raise RuntimeError('LoraSet.detach: nothing attached')
        _check_idle()
        for nm in self._nets.values():
            nm.restore()
        nets, self._nets = self._nets, None
        _refresh(self.unet, self.text_encoder, nets)


@torch.no_grad()
def fuse(unet, text_encoder, adapters, scales):
    """The permanent form: the same launch in place (base == dst), nothing saved, no state.  Allowed on a network that trains (that is
    the use: distil a fine-tune); refused on a HipControlNet and inside a grouped pass or graph capture."""
    unet = _unet_of(unet)
    _check_idle()
    scales = check_scales(scales, len(adapters))
    plans = _plans(unet, text_encoder, adapters)
    dev = unet._flat['p'].device
    done = {}
    for net, weights in (('unet', _unet_weights(unet, plans['unet'])), ('te', _te_weights(text_encoder, plans['te']) if 'te' in plans else [])):
        if net in plans and plans[net].layers:
            nm = _NetMerge(plans[net], weights, dev, False)
            nm.merge(scales)
            done[net] = nm
    torch.cuda.current_stream().synchronize()       # the factor buffers die with this call: let the launch finish first
    _refresh(unet, text_encoder, done)


def load_adapters(specs, unet, text_encoder=None, seed=0):
    """[spec] -> ([parse_lora result per spec], [notice lines]).  A spec is a local file or 'random:lora[:rank[:seed]]'."""
    adapters, notes = [], []
    for i, spec in enumerate(specs):
        name = str(spec)
        if name.lower().startswith('random:'):
            rank, s = parse_random_spec(name)
            sd = random_lora_state_dict(unet, text_encoder, rank, seed + i if s is None else s)
            notes.append(f'NOTE: {name}: seeded random LoRA factors -- images and scores from it are not comparable with any published LoRA')
        else:
            sd = read_lora_file(name)
        adapters.append(parse_lora(sd, unet, text_encoder, where=name))
    return adapters, notes
