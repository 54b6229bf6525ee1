"""fp64 restatements of sid_lsg_amd.fidelity for the tests: SSIM in its valid-window form, the sums sidlsg_psnr_ssim_u8 writes, the
LPIPS layer, and LPIPS-VGG as plain torch.nn modules that load the same state dicts through the same key names."""
import numpy as np
import torch

K1, K2, L = 0.01, 0.03, 255.0
C1, C2 = (K1 * L) ** 2, (K2 * L) ** 2
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
TAPS = (3, 8, 15, 22, 29)          # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 in torchvision's vgg16.features
VGG_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512]


def window():
    """The 11 normalised weights exp(-x^2 / (2 1.5^2)), x = -5 .. 5, fp64."""
    x = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def _filter(img):
    """[H, W] fp64 -> [H - 10, W - 10]: the separable window over every valid position, rows of the window first."""
    g = window()
    H, W = img.shape
    h = sum(g[k] * img[:, k:k + W - 10] for k in range(11))
    return sum(g[k] * h[k:k + H - 10, :] for k in range(11))


def ssim_map(x, y):
    """Two [H, W] planes (any integer or float type) -> the SSIM index of every valid 11 x 11 window, [H - 10, W - 10] fp64."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mx, my = _filter(x), _filter(y)
    vx, vy, cxy = _filter(x * x) - mx * mx, _filter(y * y) - my * my, _filter(x * y) - mx * my
    return ((2.0 * (mx * my) + C1) * (2.0 * cxy + C2)) / (((mx * mx + my * my) + C1) * ((vx + vy) + C2))


def ssim_map_scipy(x, y):
    """The same map through scipy.ndimage.gaussian_filter(sigma 1.5, truncate 3.5, reflect), cropped by 5."""
    from scipy.ndimage import gaussian_filter

    def f(a):
        return gaussian_filter(np.asarray(a, dtype=np.float64), sigma=1.5, truncate=3.5, mode='reflect')[5:-5, 5:-5]
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mx, my = f(x), f(y)
    vx, vy, cxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    return ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def psnr_ssim_sums(a, b, mask=None):
    """uint8 [B, 3, H, W] numpy a and b, mask uint8 [B, H, W] or None (all kept) -> [B, 8]: sse (int64), n, ssim_sum (fp64), ssim_n and
    the same over kept positions (mask < 128; an SSIM term is kept when its window's centre pixel is)."""
    B, _, H, W = a.shape
    out = []
    for i in range(B):
        keep = np.ones((H, W), dtype=bool) if mask is None else mask[i] < 128
        d = a[i].astype(np.int64) - b[i].astype(np.int64)
        sq = d * d
        maps = np.stack([ssim_map(a[i, c], b[i, c]) for c in range(3)])
        kc = keep[5:H - 5, 5:W - 5]
        out.append([int(sq.sum()), 3 * H * W, float(maps.sum()), 3 * (H - 10) * (W - 10),
                    int(sq[:, keep].sum()), 3 * int(keep.sum()), float(maps[:, kc].sum()), 3 * int(kc.sum())])
    return out


def lpips_layer(F, w, C):
    """F [2B, h, wd, ldf] and w [C], any float type -> (out [B], M [B]) fp64: the spatial mean of sum_c w_c (n0_c - n1_c)^2 with
    n = f / (|f|_2 + 1e-10) over the first C channels, and of sum_c |w_c| (|n0_c| + |n1_c|)^2 (the magnitude the error bound scales with)."""
    F = F.double()[..., :C]
    B = F.shape[0] // 2
    n = F / (F.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    n0, n1, w = n[:B], n[B:], w.double()
    out = (w * (n0 - n1) ** 2).sum(-1).mean(dim=(1, 2))
    mag = (w.abs() * (n0.abs() + n1.abs()) ** 2).sum(-1).mean(dim=(1, 2))
    return out, mag


class LpipsVgg(torch.nn.Module):
    """LPIPS-VGG (the lpips package v0.1, restated): `features` is torchvision's vgg16.features layout, so a torchvision state dict
    loads through its own key names; `lin{i}.model.1.weight` likewise."""

    def __init__(self):
        super().__init__()
        layers, cin = [], 3
        for v in VGG_CFG:
            if v == 'M':
                layers.append(torch.nn.MaxPool2d(2, 2))
            else:
                layers += [torch.nn.Conv2d(cin, v, 3, padding=1), torch.nn.ReLU()]
                cin = v
        self.features = torch.nn.Sequential(*layers)
        for i, c in enumerate((64, 128, 256, 512, 512)):
            lin = torch.nn.Module()
            lin.model = torch.nn.Sequential(torch.nn.Identity(), torch.nn.Conv2d(c, 1, 1, bias=False))
            setattr(self, f'lin{i}', lin)
        self.register_buffer('shift', torch.tensor(SHIFT, dtype=torch.float32)[None, :, None, None], persistent=False)
        self.register_buffer('scale', torch.tensor(SCALE, dtype=torch.float32)[None, :, None, None], persistent=False)

    def load(self, vgg_sd, lin_sd):
        missing = self.load_state_dict({**{k: v for k, v in vgg_sd.items() if k.startswith('features.')}, **lin_sd}, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        return self

    def taps(self, images_u8):
        """uint8 [B, 3, H, W] -> the five tap feature maps, NCHW, in the module's dtype."""
        dt = self.features[0].weight.dtype
        x = images_u8.to(dt) / 127.5 - 1
        x = (x - self.shift.to(dt)) / self.scale.to(dt)      # the constants are the fp32 values the kernel is handed
        out = []
        for i, m in enumerate(self.features):
            x = m(x)
            if i in TAPS:
                out.append(x)
        return out

    def tap_values(self, a_u8, b_u8):
        """-> [5, B]: the distance of every pair at every tap."""
        out = []
        for i, (f0, f1) in enumerate(zip(self.taps(a_u8), self.taps(b_u8))):
            n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            out.append(getattr(self, f'lin{i}').model((n0 - n1) ** 2).mean(dim=(1, 2, 3)))
        return torch.stack(out)

    def forward(self, a_u8, b_u8):
        return self.tap_values(a_u8, b_u8).sum(0)
