"""KID / CMMD on the GPU: sidlsg_pair_kernel_sums against the fp64 restatement of tests/test_kernel_metrics_host.py within a bound
derived from the operands, the index lists against gathered copies bit for bit, the exact zeros, determinism, the argument checks,
and metrics.compute_kid / compute_cmmd / the command line end to end.

The bound (pair_error_bound).  g = a . b comes off v_mfma_f32_16x16x4_f32 as an fp32 fma chain: |g^ - g| <= C sum_k |a_k b_k| with
C = 3.5e-7 (the chain's error up to K = 4096).  u = 2^-24 is the unit roundoff of one fp32 rounding.
  kind 0:  t = p0 g + p1 by one fma, then two products: 3 roundings.  |t^ - t| <= et = |p0| C G + u (|t| + |p0| C G);
           |v^ - v| <= 3 T^2 et + 2.01 u T^3,  T = |t| + et.
  kind 1:  the norms are chains of the same kind (error C |a|^2, C |b|^2); their sum is 1 rounding, the fma to d2 another, p0 d2 a
           third, and expm1f is taken at the 3 ulp (= 6 u relative) the OpenCL profile allows: 3 roundings and the function.
           |d2^ - d2| <= ed = C (|a|^2 + |b|^2 + 2 G) + 1.01 u (|a|^2 + |b|^2) + u (d2 + the former two)   (the clamp at 0 moves
           d2^ towards d2 >= 0); d v / d d2 = p0 exp(-p0 d2) <= p0, so |v^ - v| <= p0 ed + u p0 (d2 + ed) + 6 u (v + p0 ed).
Summed over the pairs of each quantity; the fp64 additions add at most n^2 2^-53 of the sum, counted as 2^-40 of it."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from test_kernel_metrics_host import POLY3, RBF, restate_cmmd, restate_kernel_matrix, restate_kid, restate_sums, unit_rows

pytestmark = pytest.mark.gpu

C_CHAIN, U = 3.5e-7, 2.0 ** -24
P0_RBF = float(np.float32(1.0 / 200.0))        # 1 / (2 sigma^2), sigma = 10, as the kernel receives it
QUANTITIES = ('Sxx', 'Syy', 'Sxy', 'Txx', 'Tyy')


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')


def pair_error_bound(x, y, kind, p0, p1=0.0):
    """[5] bounds on |kernel - restatement| of (Sxx, Syy, Sxy, Txx, Tyy), from the operand magnitudes (module docstring)."""
    def matrix(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        G = np.abs(a) @ np.abs(b).T
        if kind == POLY3:
            t = p0 * (a @ b.T) + p1
            et = abs(p0) * C_CHAIN * G + U * (np.abs(t) + abs(p0) * C_CHAIN * G)
            T = np.abs(t) + et
            e = 3.0 * T ** 2 * et + 2.01 * U * T ** 3
            v = np.abs(t) ** 3
        else:
            na, nb = (a * a).sum(1)[:, None], (b * b).sum(1)[None, :]
            d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
            ed = C_CHAIN * (na + nb + 2.0 * G) + 1.01 * U * (na + nb)
            ed = ed + U * (d2 + ed)
            v = -np.expm1(-p0 * d2)
            e = p0 * ed + U * p0 * (d2 + ed) + 6.0 * U * (v + p0 * ed)
        return e + 2.0 ** -40 * v
    exx, eyy, exy = matrix(x, x), matrix(y, y), matrix(x, y)
    return np.array([exx.sum(), eyy.sum(), exy.sum(), np.trace(exx), np.trace(eyy)])


def _data(kind, n, F, seed, shift=0.0):
    rs = np.random.RandomState(seed)
    if kind == RBF:
        return unit_rows(rs, n, F, shift)
    return (np.abs(rs.randn(n, F)) * 0.7 + shift).astype(np.float32)         # Inception pool features are non-negative


def _params(kind, F):
    return (float(np.float32(1.0 / F)), 1.0) if kind == POLY3 else (P0_RBF, 0.0)


def _run(x, y, kind, p0, p1, ix=None, iy=None):
    from sid_lsg_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    return ops.pair_kernel_sums(t(x), t(y), kind, p0, p1, t(ix), t(iy))


# |kernel - restatement| as measured on an MI355X, per case and kind, in the order of QUANTITIES: the test asserts the derived bound
# and 4 x these, whichever is smaller
MEASURED = {
    (5, 3, 4, 0): [3.729e-07, 1.678e-07, 1.045e-06, 1.377e-06, 1.946e-06],
    (5, 3, 4, 1): [6.660e-10, 8.839e-10, 2.378e-09, 0.000e+00, 0.000e+00],
    (130, 131, 36, 0): [2.209e-04, 6.936e-04, 3.563e-04, 2.192e-06, 5.708e-06],
    (130, 131, 36, 1): [2.735e-06, 1.858e-06, 2.199e-06, 0.000e+00, 0.000e+00],
    (257, 3, 68, 0): [6.571e-04, 3.225e-06, 1.921e-05, 1.555e-07, 7.449e-07],
    (257, 3, 68, 1): [1.098e-06, 2.561e-09, 1.561e-07, 0.000e+00, 0.000e+00],
    (257, 131, 68, 0): [6.571e-04, 5.008e-05, 3.500e-04, 1.555e-07, 2.007e-05],
    (257, 131, 68, 1): [1.098e-06, 1.081e-06, 1.327e-06, 0.000e+00, 0.000e+00],
}

# x (n, F) against y (n, F): below a tile; one row past a tile against one more (mx != my, F = 32 + 4); three row tiles against a
# sliver and against two tiles (the upper-triangle walk, the x2 weight, a partly filled last diagonal tile; F = 64 + 4)
SHAPES = [(5, 3, 4), (130, 131, 36), (257, 3, 68), (257, 131, 68)]


@pytest.mark.parametrize('kind', [POLY3, RBF])
@pytest.mark.parametrize('nx,ny,F', SHAPES)
def test_sums_match_the_restatement(nx, ny, F, kind):
    """All five sums within the derived bound.  A kernel that counts the zero rows a tile is padded with is off by whole units in
    the polynomial kind ((0 + 1)^3 = 1 per padded pair) and by about 0.01 per pair in the RBF kind."""
    _need_gpu()
    x, y = _data(kind, nx, F, 10 + nx), _data(kind, ny, F, 20 + ny, shift=0.25)
    p0, p1 = _params(kind, F)
    got = _run(x, y, kind, p0, p1)
    assert got.shape == (1, 5) and got.dtype == torch.float64
    got = got.cpu().numpy()[0]
    want, bound = restate_sums(x, y, kind, p0, p1), pair_error_bound(x, y, kind, p0, p1)
    err = np.abs(got - want)
    print(f'MEASURED ({nx}, {ny}, {F}, {kind}): [' + ', '.join(f'{e:.3e}' for e in err) + '],')
    print('   bound [' + ', '.join(f'{b:.3e}' for b in bound) + ']  sums [' + ', '.join(f'{w:.6e}' for w in want) + ']')
    measured = MEASURED.get((nx, ny, F, kind))
    limit = bound if measured is None else np.minimum(bound, 4.0 * np.asarray(measured))
    for q, e, lim in zip(QUANTITIES, err, limit):
        assert e <= lim, f'{q}: |kernel - restatement| = {e:.3e} > {lim:.3e}'


@pytest.mark.parametrize('kind', [POLY3, RBF])
def test_index_lists_equal_gathered_copies_bit_for_bit(kind):
    """S = 3 subsets of m = 130 of n = 200 rows, ONE matrix passed as both X and Y: subset 1 shares a row with subset 0, subset 2
    uses the same list on both sides.  Equal to the kernel on explicitly gathered copies bit for bit, and to the restatement."""
    _need_gpu()
    n, F, m = 200, 36, 130
    x = _data(kind, n, F, 5)
    rs = np.random.RandomState(6)
    ix = np.stack([rs.choice(n, m, replace=False) for _ in range(3)]).astype(np.int32)
    iy = np.stack([rs.choice(n, m, replace=False) for _ in range(3)]).astype(np.int32)
    ix[1, 0] = ix[0, 0] if ix[0, 0] not in ix[1] else ix[1, 0]
    assert set(ix[0]) & set(ix[1])
    iy[2] = ix[2]
    p0, p1 = _params(kind, F)
    from sid_lsg_amd import ops
    xt = torch.from_numpy(x).cuda()
    got = ops.pair_kernel_sums(xt, xt, kind, p0, p1, torch.from_numpy(ix).cuda(), torch.from_numpy(iy).cuda())
    assert got.shape == (3, 5)
    for s in range(3):
        gathered = _run(x[ix[s]], x[iy[s]], kind, p0, p1)
        assert torch.equal(got[s], gathered[0]), f'subset {s}: {got[s].tolist()} vs gathered {gathered[0].tolist()}'
        want, bound = restate_sums(x[ix[s]], x[iy[s]], kind, p0, p1), pair_error_bound(x[ix[s]], x[iy[s]], kind, p0, p1)
        err = np.abs(got[s].cpu().numpy() - want)
        print(f'subset {s} kind {kind}: err [' + ', '.join(f'{e:.3e}' for e in err) + '] bound [' + ', '.join(f'{b:.3e}' for b in bound) + ']')
        assert (err <= bound).all()
    g2 = got[2].cpu().numpy()
    assert abs(g2[2] - g2[0]) <= 1e-12 * abs(g2[0]) and g2[3] == g2[4]       # the same pairs, added in another order


def test_rows_past_two_gib_are_addressed():
    """A feature matrix of 2 GiB + 4 KiB: the rows an index list picks behind the 2^31-byte mark (element offsets past 2^29) are the
    rows the kernel reads -- equal to the kernel on a gathered copy bit for bit."""
    _need_gpu()
    from sid_lsg_amd import ops
    F = 512
    n = (1 << 31) // (4 * F) + 2
    x = torch.zeros((n, F), device='cuda')
    g = torch.Generator(device='cuda').manual_seed(9)
    rows = torch.tensor([n - 1, 0, n - 2, n // 2 + 1], device='cuda')
    x[rows] = torch.randn((4, F), device='cuda', generator=g).abs()
    idx = rows.int()[None]
    got = ops.pair_kernel_sums(x, x, POLY3, 1.0 / F, 1.0, idx, idx.flip(1))
    small = x[rows].contiguous()
    assert torch.equal(got, ops.pair_kernel_sums(small, small.flip(0).contiguous(), POLY3, 1.0 / F, 1.0))
    assert float(got[0, 0]) > 16.0          # zero rows would give exactly 16 pairs of (0 + 1)^3


def test_rbf_exact_zeros():
    """A row against itself or a bit-identical duplicate has d2 == 0: Txx == 0.0 exactly, duplicates or not.  A set against itself:
    Sxy is Sxx up to the order of the fp64 additions."""
    _need_gpu()
    x = _data(RBF, 150, 36, 7)
    x[140:] = x[:10]                                   # duplicates in another tile
    x[20:25] = x[30:35]                                # and within one
    got = _run(x, x, RBF, P0_RBF, 0.0).cpu().numpy()[0]
    assert got[3] == 0.0 and got[4] == 0.0
    assert got[0] > 0 and abs(got[2] - got[0]) <= 1e-12 * got[0] and got[1] == got[0]
    # the duplicated pairs contribute exactly nothing: removing the duplicates' mutual pairs from the restatement is not needed,
    # their v is 0 there as well; the sums agree within the bound
    assert (np.abs(got - restate_sums(x, x, RBF, P0_RBF)) <= pair_error_bound(x, x, RBF, P0_RBF)).all()


def test_rbf_cancellation_stays_non_negative():
    """Rows of norm about 1e3 that differ in their last bits: |a|^2 + |b|^2 - 2 a.b cancels to rounding noise of either sign; the
    clamp keeps d2 >= 0, so every v lies in [0, 1]: finite sums, none negative, none above the pair count."""
    _need_gpu()
    rs = np.random.RandomState(8)
    base = rs.randn(36).astype(np.float32)
    base *= np.float32(1e3) / np.linalg.norm(base)
    x = np.tile(base, (40, 1))
    flip = rs.randint(0, 2, x.shape).astype(bool)
    x = np.where(flip, np.nextafter(x, np.float32(np.inf)), x).astype(np.float32)
    got = _run(x, x, RBF, P0_RBF, 0.0).cpu().numpy()[0]
    assert np.isfinite(got).all() and (got >= 0).all() and (got[:3] <= 40 * 40).all() and got[3] == 0.0 and got[4] == 0.0


@pytest.mark.parametrize('kind', [POLY3, RBF])
def test_two_runs_give_the_same_bits(kind):
    _need_gpu()
    x, y = _data(kind, 257, 68, 267), _data(kind, 131, 68, 151, shift=0.25)
    p0, p1 = _params(kind, 68)
    assert torch.equal(_run(x, y, kind, p0, p1), _run(x, y, kind, p0, p1))


def test_arguments_are_checked():
    _need_gpu()
    from sid_lsg_amd import ops
    x = torch.randn(64, 8, device='cuda')
    idx = torch.zeros((2, 5), dtype=torch.int32, device='cuda')
    out = torch.full((2, 5), 7.0, dtype=torch.float64, device='cuda')
    ws = torch.zeros(64, dtype=torch.float64, device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    call = lambda F, ix, iy, S, mx, my, kind: ops.lib.sidlsg_pair_kernel_sums(      # noqa: E731
        x.data_ptr(), 64, x.data_ptr(), 64, F, ix, iy, S, mx, my, kind, 1.0, 1.0, out.data_ptr(), ws.data_ptr(), s)
    i = idx.data_ptr()
    for args in ((6, i, i, 2, 5, 5, 0), (8, i, None, 2, 5, 5, 0), (8, i, i, 2, 5, 5, 2), (8, i, i, 0, 5, 5, 0), (8, i, i, 2, 0, 5, 0),
                 (8, None, None, 2, 64, 64, 0), (8, None, None, 1, 5, 64, 0)):
        with pytest.raises(RuntimeError, match='failed with code -22'):
            call(*args)
    assert ops.lib.sidlsg_pair_kernel_sums_ws_doubles.raw(0, 5, 5) < 0 and ops.lib.sidlsg_pair_kernel_sums_ws_doubles.raw(2, 5, 5) == 2 * 2 * 3
    with pytest.raises(RuntimeError):
        ops.pair_kernel_sums(x, x, 0, 1.0, 1.0, idx_x=idx)                        # one-sided index list
    with pytest.raises(RuntimeError):
        ops.pair_kernel_sums(x, x, 2, 1.0, 1.0)                                   # kind
    with pytest.raises(RuntimeError):
        ops.pair_kernel_sums(x, x, 0, 1.0, 1.0, idx[:0], idx[:0])                 # S = 0
    with pytest.raises(RuntimeError):
        ops.pair_kernel_sums(x, x, 0, 1.0, 1.0, idx + 64, idx)                    # an index past the last row
    with pytest.raises(RuntimeError):
        ops.pair_kernel_sums(x, x.double(), 0, 1.0, 1.0)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), 'nothing was launched'
    # F = 6 through ops is padded to 8 with zero columns, which change no dot product
    a = ops.pair_kernel_sums(x[:, :6].contiguous(), x[:, :6].contiguous(), 0, 0.125, 1.0)
    b = ops.pair_kernel_sums(torch.nn.functional.pad(x[:, :6], [0, 2]), torch.nn.functional.pad(x[:, :6], [0, 2]), 0, 0.125, 1.0)
    assert torch.equal(a, b)


# ---- end to end ------------------------------------------------------------------------------------------------------------
class _Images:
    """An in-memory image set with the dataset item contract: uint8 [3, H, W] images (one of them not square) and captions."""
    has_images = True

    def __init__(self, n, size, hi, seed):
        rs = np.random.RandomState(seed)
        self.images = [torch.from_numpy(rs.randint(0, hi, (3, size, size if i != 2 else size - 16)).astype(np.uint8)) for i in range(n)]

    def __len__(self):
        return len(self.images)

    def caption(self, i):
        return f'caption {i}'

    def __getitem__(self, i):
        return self.images[i], self.caption(i)


def _bright_generator(latents, contexts, init_timesteps=None):
    z = torch.nn.functional.interpolate(latents[:, :3], size=(64, 64), mode='nearest')
    return torch.tanh(z) * 0.4 + 0.6            # seeded by the latents; [0.2, 1]: far from the dark real images


def _grid_detector(images, return_features=True):
    """16 features per image: the 4 x 4 grid of block means of channel 0, cut to multiples of 1/16 below 4."""
    pooled = torch.nn.functional.adaptive_avg_pool2d(images[:, :1].float(), 4).flatten(1)
    return torch.floor(pooled / 4.0) / 16.0


def test_compute_kid_end_to_end():
    """compute_kid with a callable detector and a callable G, against the restatement on the features the same functions capture.
    Relative 1e-6: the detector's features are multiples of 1/16 below 4, so every product (a multiple of 1/256 below 16), every
    partial sum of the 16 (below 256: 16 bits) and t = g / 16 + 1 (a multiple of 2^-12 below 17: 17 bits) is an fp32 number: the
    chain and the fma are exact, and v carries the 2 roundings of its two products, |v^ - v| <= 2.01 u v.  Through the estimator
    that is 2.01 u (sum_{i != j} (kxx + kyy) / (m - 1) + 2 sum kxy / m) / m per subset, which the test evaluates and finds below
    1e-6 of the KID of these two very different sets before it asserts 1e-6."""
    _need_gpu()
    from sid_lsg_amd import metrics
    opts = metrics.MetricOptions(G=_bright_generator, dataset=_Images(20, 64, 64, 3), detector=_grid_detector, device='cuda', resolution=64, batch_gen=8)
    S, cap, num_gen = 4, 16, 24
    got = metrics.compute_kid(opts, max_real=None, num_gen=num_gen, num_subsets=S, max_subset_size=cap)
    real = metrics.dataset_feature_stats(opts, capture_all=True).get_all_torch().cpu().numpy()
    gen = metrics.generator_feature_stats(opts, num_gen, capture_all=True)[0].get_all_torch().cpu().numpy()
    assert real.shape == (20, 16) and gen.shape == (num_gen, 16) and real.dtype == np.float32
    assert (real * 16 == np.round(real * 16)).all() and (gen * 16 == np.round(gen * 16)).all() and max(real.max(), gen.max()) < 4
    ix, iy = metrics.kid_subsets(num_gen, 20, S, cap, seed=0)
    m = ix.shape[1]
    want = restate_kid(gen, real, ix, iy)
    derived = 0.0
    for sx, sy in zip(ix, iy):
        kxx, kyy, kxy = (restate_kernel_matrix(a, b, POLY3, 1.0 / 16, 1.0) for a, b in ((gen[sx], gen[sx]), (real[sy], real[sy]), (gen[sx], real[sy])))
        derived += 2.01 * U * ((kxx.sum() - np.trace(kxx) + kyy.sum() - np.trace(kyy)) / (m - 1) + 2.0 * kxy.sum() / m) / m / S
    print(f'KID {got:.12e}, restatement {want:.12e}, |difference| {abs(got - want):.3e}, derived bound {derived:.3e}')
    assert derived <= 1e-6 * abs(want)
    assert abs(got - want) <= 1e-6 * abs(want)


def test_compute_cmmd_end_to_end():
    """compute_cmmd with random:clip-tiny (32 x 32 input, patch 8), a seeded G and a small image set with one image that is not
    square, against the restatement on the embeddings the same functions capture.  Absolute 1e-4 in the x 1000 units: for unit
    rows |a|^2 + |b|^2 + 2 G <= 4 and d2 <= 4, so ed <= 3.5e-7 * 4 + 2.02 u + 4 u < 1.8e-6 and, with p0 = 1 / 200 and v <= 0.02,
    |v^ - v| <= 9e-9 + 1.2e-9 + 7.3e-9 < 1.8e-8 for every pair; the three means enter with weights 2, 1, 1: 4 * 1.8e-8 * 1000 =
    7.2e-5.  The test evaluates pair_error_bound on the captured embeddings and checks that it stays below 1e-4 first."""
    _need_gpu()
    from sid_lsg_amd import metrics
    opts = metrics.MetricOptions(G=_bright_generator, dataset=_Images(9, 48, 256, 4), device='cuda', resolution=64, batch_gen=4,
                                 metric_cmmd_clip_path='random:clip-tiny')
    num_gen = 10
    got = metrics.compute_cmmd(opts, max_real=None, num_gen=num_gen)
    o = metrics.cmmd_options(opts)
    real = metrics.dataset_feature_stats(o, capture_all=True).get_all_torch().cpu().numpy()
    gen = metrics.generator_feature_stats(o, num_gen, capture_all=True)[0].get_all_torch().cpu().numpy()
    assert real.shape == (9, 32) and gen.shape == (num_gen, 32) and real.dtype == np.float32
    assert np.abs(np.linalg.norm(np.concatenate([real, gen]).astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    want = restate_cmmd(real, gen)
    b = pair_error_bound(real, gen, RBF, P0_RBF)
    derived = 1000.0 * (2.0 * b[2] / (9 * num_gen) + b[0] / 81 + b[1] / num_gen ** 2)
    # the kernel's p0 is 1 / 200 rounded to fp32, the restatement's is not: a relative u on every exponent p0 d2 <= 0.02
    derived += 1000.0 * 4.0 * U * P0_RBF * 4.0
    print(f'CMMD {got:.9e}, restatement {want:.9e}, |difference| {abs(got - want):.3e}, derived bound {derived:.3e}')
    assert derived <= 1e-4
    assert np.isfinite(got) and abs(got - want) <= 1e-4


def test_image_set_distance_tool_scores_two_folders(tmp_path):
    """tools/image_set_distance.py --cmmd on two folders (one image not square): the number cmmd_from_features gives for the
    embeddings of the same files, and different folders are apart while a folder against itself is at 0."""
    _need_gpu()
    import importlib.util
    import PIL.Image
    from sid_lsg_amd import metrics
    spec = importlib.util.spec_from_file_location('image_set_distance', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                     'tools', 'image_set_distance.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rs = np.random.RandomState(12)
    for name, lo, hi in (('real', 0, 128), ('fake', 100, 256)):
        (tmp_path / name).mkdir()
        for i in range(6):
            arr = rs.randint(lo, hi, (40, 24 if i == 3 else 40, 3)).astype(np.uint8)
            PIL.Image.fromarray(arr).save(str(tmp_path / name / f'{i:06d}.png'))
    res = tool.main(['--real', str(tmp_path / 'real'), '--fake', str(tmp_path / 'fake'), '--cmmd', '--clip', 'random:clip-tiny', '--batch', '4'])
    det = metrics.ClipEmbeddingDetector('random:clip-tiny', 'cuda')
    feats = [tool.features(tool.image_files(str(tmp_path / n)), det, torch.device('cuda'), 4) for n in ('real', 'fake')]
    assert feats[0].shape == (6, 32) and res['cmmd'] > 0
    assert abs(res['cmmd'] - restate_cmmd(feats[0].cpu().numpy(), feats[1].cpu().numpy())) <= 1e-4       # the bound of test_compute_cmmd_end_to_end
    # a set against itself: Sxx = Syy = Sxy up to the order of the fp64 additions (1e-12 relative of sums below 1)
    assert abs(metrics.cmmd_from_features(feats[0], feats[0])) <= 1e-9
    with pytest.raises(SystemExit):
        tool.main(['--real', str(tmp_path / 'real'), '--fake', str(tmp_path / 'fake')])


def test_cli_writes_both_metric_lines(tmp_path):
    """sid_train.py --train_mode 0 --network_pkl teacher --metrics kid_test,cmmd_test on random:tiny: one report line each.  The
    _test forms generate ONE image (the count of fid_test / pr_test), which leaves KID without a pair: NaN; CMMD is a number."""
    _need_gpu()
    import PIL.Image
    from click.testing import CliRunner
    import sid_train

    class Detector(torch.nn.Module):        # the stand-in of tests/test_gpu_cli.py::test_train_with_fid_metric
        def __init__(self):
            super().__init__()
            torch.manual_seed(0)
            self.conv = torch.nn.Conv2d(3, 16, 8, stride=8)

        def forward(self, img: torch.Tensor, return_features: bool = True) -> torch.Tensor:
            return self.conv(img.to(torch.float32) / 255.0).mean(dim=(2, 3))
    det_path = str(tmp_path / 'detector.pt')
    torch.jit.script(Detector()).save(det_path)
    (tmp_path / 'aesthetics_6_plus.txt').write_text('\n'.join(f'prompt number {i}' for i in range(40)) + '\n')
    data = tmp_path / 'coco'
    data.mkdir()
    rs = np.random.RandomState(11)
    for i in range(5):
        PIL.Image.fromarray(rs.randint(0, 256, (64, 48 if i == 1 else 64, 3)).astype(np.uint8)).save(str(data / f'img_{i}.png'))
        (data / f'img_{i}.txt').write_text(f'evaluation caption {i}\n')
    runs = tmp_path / 'runs'
    ev = CliRunner().invoke(sid_train.main, [
        '--outdir', str(runs), '--data_prompt_text', str(tmp_path), '--data', str(data), '--sd_model', 'random:tiny', '--seed', '1',
        '--resolution', '64', '--batch', '8', '--batch-gpu', '8', '--train_mode', '0', '--network_pkl', 'teacher', '--teacher_steps', '2',
        '--teacher_cfg', '2', '--metrics', 'kid_test,cmmd_test', '--metric_pt_path', det_path, '--metric_cmmd_clip_path', 'random:clip-tiny'],
        catch_exceptions=False)
    assert ev.exit_code == 0, ev.output
    run_dir = glob.glob(str(runs / '00000-*'))[0]
    kid = [json.loads(ln) for ln in open(os.path.join(run_dir, 'metric-kid_test.jsonl'))]
    cmmd = [json.loads(ln) for ln in open(os.path.join(run_dir, 'metric-cmmd_test.jsonl'))]
    assert len(kid) == 1 and kid[0]['metric'] == 'kid_test' and np.isnan(kid[0]['results']['kid30k_full'])
    assert len(cmmd) == 1 and cmmd[0]['metric'] == 'cmmd_test' and np.isfinite(cmmd[0]['results']['cmmd30k_full'])
    assert cmmd[0]['results']['cmmd30k_full'] > -1e-4
    assert json.load(open(os.path.join(run_dir, 'training_options.json')))['metric_cmmd_clip_path'] == 'random:clip-tiny'
