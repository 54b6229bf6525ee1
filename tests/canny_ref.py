"""An independent restatement of the Canny / edge-matching rules of include/sidlsg_hip.h for the tests: a plain per-pixel loop for
classify, scipy.ndimage.label (full 3 x 3 structure) for the hysteresis, scipy.ndimage.binary_dilation for D_r.  numpy / scipy only:
nothing here touches the package's kernels or its bit planes."""
import numpy as np
from scipy import ndimage

TG22 = 13573
FULL = np.ones((3, 3), dtype=bool)


def sobel_ref(img):
    """uint8 [H, W, 3] -> (dx, dy, m) int [H, W]: per-channel 3 x 3 Sobel on the replicated border, the channel of the largest
    |dx| + |dy| (the first on a tie)."""
    H, W, _ = img.shape
    p = np.pad(img.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode='edge')
    dx, dy, m = (np.zeros((H, W), dtype=np.int64) for _ in range(3))
    for y in range(H):
        for x in range(W):
            best = -1
            for c in range(3):
                q = p[y:y + 3, x:x + 3, c]
                cdx = (q[0, 2] + 2 * q[1, 2] + q[2, 2]) - (q[0, 0] + 2 * q[1, 0] + q[2, 0])
                cdy = (q[2, 0] + 2 * q[2, 1] + q[2, 2]) - (q[0, 0] + 2 * q[0, 1] + q[0, 2])
                if abs(cdx) + abs(cdy) > best:
                    best, dx[y, x], dy[y, x] = abs(cdx) + abs(cdy), cdx, cdy
            m[y, x] = best
    return dx, dy, m


def classify_ref(img, low=100, high=200):
    """uint8 [H, W, 3] -> (cand, strong) bool [H, W], and the magnitude map."""
    H, W, _ = img.shape
    dx, dy, m = sobel_ref(img)
    mp = np.pad(m, 1)                                  # the magnitude outside the image is 0
    cand, strong = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            v = int(m[y, x])
            if not v > low:
                continue
            M = lambda yy, xx: int(mp[yy + 1, xx + 1])  # noqa: E731
            ax, ay = abs(int(dx[y, x])), abs(int(dy[y, x])) << 15
            t22 = ax * TG22
            t67 = t22 + (ax << 16)
            if ay < t22:
                keep = v > M(y, x - 1) and v >= M(y, x + 1)
            elif ay > t67:
                keep = v > M(y - 1, x) and v >= M(y + 1, x)
            else:
                s = -1 if (int(dx[y, x]) ^ int(dy[y, x])) < 0 else 1
                keep = v > M(y - 1, x - s) and v > M(y + 1, x + s)
            cand[y, x] = keep
            strong[y, x] = keep and v > high
    return cand, strong, m


def hysteresis_ref(cand, strong):
    """bool [H, W] -> the candidate components (8-connectivity) that contain a strong candidate."""
    lab, n = ndimage.label(cand, structure=FULL)
    keep = np.zeros(n + 1, dtype=bool)
    keep[np.unique(lab[strong & cand])] = True
    keep[0] = False
    return keep[lab]


def canny_ref(img, low=100, high=200):
    cand, strong, _ = classify_ref(img, low, high)
    return hysteresis_ref(cand, strong)


def dilate_ref(a, r):
    return a.copy() if r == 0 else ndimage.binary_dilation(a, structure=FULL, iterations=r)


def match_ref(a, b, r):
    """bool [H, W] a, b -> [|a|, |b|, |a & D_r(b)|, |b & D_r(a)|]."""
    return [int(a.sum()), int(b.sum()), int((a & dilate_ref(b, r)).sum()), int((b & dilate_ref(a, r)).sum())]


def geodesic_depth(cand, strong):
    """The number of 3 x 3 dilation steps inside `cand` that the strong seeds need to reach the last pixel they reach."""
    e, n = strong & cand, 0
    while True:
        g = e | (cand & ndimage.binary_dilation(e, structure=FULL))
        if (g == e).all():
            return n
        e, n = g, n + 1


def smoothed_noise(H, W, sigma, seed):
    """The issue's recipe: Gaussian-smoothed normal noise, scaled to its own min / max, times 255, rounded -> uint8 [H, W, 3]."""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((H, W, 3)), (sigma, sigma, 0))
    return np.round((f - f.min()) / (f.max() - f.min()) * 255).astype(np.uint8)


# ---- hand-made cases (tests/test_canny_host.py states what each must give) ----
def step_edge(H=8, W=8, x0=4, lo=0, hi=200):
    """Columns < x0 at `lo`, the rest at `hi`, all channels: the magnitude is equal on columns x0 - 1 and x0, a two-pixel plateau."""
    img = np.full((H, W, 3), lo, dtype=np.uint8)
    img[:, x0:] = hi
    return img


def blue_only_edge(H=8, W=8, y0=4):
    """A horizontal step present in channel B only."""
    img = np.zeros((H, W, 3), dtype=np.uint8)
    img[y0:, :, 2] = 220
    return img


def serpentine(n=64, gap=None):
    """cand: even rows full, joined alternately at the right and left ends through the odd rows; strong: the pixel (0, 0).  `gap`: one
    (y, x) removed from cand."""
    cand = np.zeros((n, n), dtype=bool)
    cand[0::2] = True
    for k, y in enumerate(range(1, n - 1, 2)):
        cand[y, n - 1 if k % 2 == 0 else 0] = True
    strong = np.zeros((n, n), dtype=bool)
    strong[0, 0] = True
    if gap is not None:
        cand[gap] = False
    return cand, strong
