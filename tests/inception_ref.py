"""A plain torch.nn restatement of the FID Inception-v3 (the pytorch-fid variant table) for the Inception tests: explicit
BatchNorm2d(eps=1e-3) in eval mode, torchvision key names, the affine_grid / grid_sample preprocessing of the published TorchScript
detector, and the seeded initialiser.  Runs on the CPU in fp32 and fp64.  Nothing here is shared with sid_lsg_amd.inception."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=1e-3)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


def _avg(x):
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, kernel_size=1)

    def forward(self, x):
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))), self.branch_pool(_avg(x))], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        return torch.cat([self.branch3x3(x), self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))), F.max_pool2d(x, 3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_5(self.branch7x7dbl_4(self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x)))))
        return torch.cat([self.branch1x1(x), b7, bd, self.branch_pool(_avg(x))], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), b7, F.max_pool2d(x, 3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin, pool):
        super().__init__()
        self.pool = pool           # 'avg' (Mixed_7b) or 'max' (Mixed_7c: the FID variant)
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b3 = self.branch3x3_1(x)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        pooled = _avg(x) if self.pool == 'avg' else F.max_pool2d(x, 3, stride=1, padding=1)
        return torch.cat([self.branch1x1(x), self.branch3x3_2a(b3), self.branch3x3_2b(b3), self.branch3x3dbl_3a(bd), self.branch3x3dbl_3b(bd),
                          self.branch_pool(pooled)], 1)


def resize_299(images):
    """uint8 (or float) NCHW -> float NCHW 299 x 299 in the dtype of the computation, as the TorchScript detector resizes: an
    affine_grid with the +1/W - 1/299 shift, then grid_sample(bilinear, border, align_corners=False)."""
    B, C, H, W = images.shape
    theta = torch.eye(2, 3, dtype=images.dtype, device=images.device)
    theta[0, 2] += theta[0, 0] / W - theta[0, 0] / 299
    theta[1, 2] += theta[1, 1] / H - theta[1, 1] / 299
    grid = F.affine_grid(theta.unsqueeze(0).repeat(B, 1, 1), [B, C, 299, 299], align_corners=False)
    return F.grid_sample(images, grid, mode='bilinear', padding_mode='border', align_corners=False)


def legacy_tf_resize_299(images_u8):
    """The same resize written out in fp64 (TF's legacy bilinear rule): source coordinate i * W / 299 exactly, taps floor and + 1
    clamped to the border, horizontal then vertical.  uint8 NCHW -> fp64 NCHW, not yet normalised."""
    x = torch.as_tensor(images_u8).double()
    H, W = x.shape[-2:]

    def taps(size):
        p = np.arange(299, dtype=np.int64) * size
        q = p // 299
        return torch.from_numpy(q), torch.from_numpy(np.minimum(q + 1, size - 1)), torch.from_numpy((p - q * 299) / 299.0)
    x0, x1, lx = taps(W)
    y0, y1, ly = taps(H)
    rows = x[..., x0] + lx * (x[..., x1] - x[..., x0])
    return rows[..., y0, :] + ly[:, None] * (rows[..., y1, :] - rows[..., y0, :])


class InceptionV3Ref(nn.Module):
    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, 'avg')
        self.Mixed_7c = InceptionE(2048, 'max')
        self.fc = nn.Linear(2048, 1008)
        self.eval().requires_grad_(False)

    def trunk(self, x):
        """Normalised 299 x 299 NCHW -> [B, 2048]."""
        x = self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x)))
        x = F.max_pool2d(x, 3, stride=2)
        x = self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x))
        x = F.max_pool2d(x, 3, stride=2)
        for name in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e', 'Mixed_7a', 'Mixed_7b', 'Mixed_7c'):
            x = getattr(self, name)(x)
        return x.mean(dim=(2, 3))

    def forward(self, images_u8, return_features=False, no_output_bias=False):
        dtype = self.fc.weight.dtype
        x = (resize_299(images_u8.to(dtype)) - 128) / 128
        f = self.trunk(x)
        if return_features:
            return f
        logits = F.linear(f, self.fc.weight, None if no_output_bias else self.fc.bias)
        return torch.softmax(logits, dim=1)


def seed_weights(net, seed=0):
    """conv N(0, 2 / fan_in); BatchNorm weight U(0.5, 1.5), bias 0.1 N, running mean 0.1 N, running var U(0.5, 1.5); fc N(0, 1 / 2048),
    bias 0.1 N.  Keeps the activations of every depth alive."""
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, nn.Conv2d):
            fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / fan_in))
        elif isinstance(m, nn.BatchNorm2d):
            m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
            m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
        elif isinstance(m, nn.Linear):
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(1.0 / m.in_features))
            m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    return net


def seeded_net(seed=0):
    with torch.no_grad():
        return seed_weights(InceptionV3Ref(), seed)


def structured_images(B, H, W, seed=0):
    """uint8 [B, 3, H, W]: coloured blocks plus noise, different per image (pure noise images sit within 1-2 % of each other in
    feature space)."""
    rs = np.random.RandomState(seed)
    img = np.zeros((B, 3, H, W), dtype=np.float64)
    for b in range(B):
        img[b] = rs.randint(0, 256, (3, 1, 1))
        for _ in range(6):
            y0, x0 = rs.randint(0, H), rs.randint(0, W)
            y1, x1 = rs.randint(y0 + 1, H + 1), rs.randint(x0 + 1, W + 1)
            img[b, :, y0:y1, x0:x1] = rs.randint(0, 256, (3, 1, 1))
    img += rs.normal(0, 12, img.shape)
    return torch.from_numpy(np.clip(np.rint(img), 0, 255).astype(np.uint8))


def rel_l2(got, want):
    """Per-row relative l2 error of [B, ...] against the fp64 `want`."""
    got, want = torch.as_tensor(got).double().flatten(1), torch.as_tensor(want).double().flatten(1)
    return ((got - want).norm(dim=1) / want.norm(dim=1)).numpy()
