"""Golden vectors of the snapshot preview grids.  AUTHORING ONLY: needs the reference checkout (and Pillow, which its loop imports).

    python tools/make_preview_goldens.py      -> tests/golden/preview_grid.npz

Both parts call the UNMODIFIED reference functions (oracle.ref_harness imports the reference in place):
  (a) setup_snapshot_image_grid on a stand-in dataset whose items name their own index, for resolutions 256 / 512 / 768 / 4096 and
      5 / 1000 items:  setup_<res>_<n>_size = (gw, gh), setup_<res>_<n>_indices = the dataset index of every tile.
  (b) save_image_grid on `images` [28, 3, 16, 16] fp32 for the dranges [-1, 1] and [0, 255], the PNG it wrote read back:
      grid_m1_1, grid_0_255 = uint8 [4 * 16, 7 * 16, 3].  `images` holds, in this order: the exact ties k + 0.5 (k = 0 .. 255) that
      decide half-to-even under [0, 255]; the values that land on ties under [-1, 1]; values below lo and above hi, +-0, denormals,
      +-inf and the largest finite values; then a seeded random bulk (half of it spread over [-1.2, 1.2], half over [-20, 280]).
      No NaN: numpy's float -> uint8 cast of NaN is undefined.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'preview_grid.npz')
RESOLUTIONS, SIZES = (256, 512, 768, 4096), (5, 1000)
GRID, TILE = (7, 4), 16


class _IndexDataset:
    """(image, context) items that carry their own index."""

    def __init__(self, n, resolution):
        self.n, self.resolution = n, resolution

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return np.array([i], dtype=np.int64), str(i)


def make_images():
    f32 = np.float32
    ties = np.arange(256, dtype=f32) + f32(0.5)
    k = np.arange(256, dtype=np.float64)
    ties_m1_1 = ((k + 0.5) / 127.5 - 1.0).astype(f32)
    tiny = np.finfo(f32).tiny
    special = np.array([0.0, -0.0, 1e-40, -1e-40, tiny, -tiny, np.inf, -np.inf, np.finfo(f32).max, np.finfo(f32).min, -0.5, -1.0, -1.5,
                        255.5, 256.5, 300.0, 1e30, -1e30, 1.0, -1.0000001, 1.0000001, 0.99607843, -3.0, 3.0, 254.5, 255.0, 127.5, 128.5],
                       dtype=f32)
    n = GRID[0] * GRID[1] * 3 * TILE * TILE
    rng = np.random.RandomState(7)
    rest = n - ties.size - ties_m1_1.size - special.size
    bulk = np.concatenate([rng.uniform(-1.2, 1.2, rest // 2), rng.uniform(-20, 280, rest - rest // 2)]).astype(f32)
    flat = np.concatenate([ties, ties_m1_1, special, bulk])
    assert flat.size == n and not np.isnan(flat).any()
    return flat.reshape(GRID[0] * GRID[1], 3, TILE, TILE)


def main():
    import PIL.Image
    ref = ref_harness.import_reference()
    out = {}
    for res in RESOLUTIONS:
        for n in SIZES:
            size, images, contexts = ref.loop.setup_snapshot_image_grid(training_set=_IndexDataset(n, res))
            idx = images[:, 0]
            assert [str(i) for i in idx] == list(contexts)
            out[f'setup_{res}_{n}_size'] = np.array([int(size[0]), int(size[1])], dtype=np.int64)
            out[f'setup_{res}_{n}_indices'] = idx.astype(np.int64)
    images = make_images()
    out['images'] = images
    with tempfile.TemporaryDirectory() as tmp:
        for key, drange in (('grid_m1_1', [-1, 1]), ('grid_0_255', [0, 255])):
            path = os.path.join(tmp, key + '.png')
            with np.errstate(all='ignore'):
                ref.loop.save_image_grid(img=images, fname=path, drange=drange, grid_size=GRID)
            out[key] = np.asarray(PIL.Image.open(path).convert('RGB'))
            assert out[key].shape == (GRID[1] * TILE, GRID[0] * TILE, 3) and out[key].dtype == np.uint8
    # the fixture means what it should: half-to-even on the ties of [0, 255] (tile 0 holds them from its first byte on)
    first = out['grid_0_255'][:TILE, :TILE].transpose(2, 0, 1).reshape(-1)[:256]
    want = np.minimum(np.where(np.arange(256) % 2 == 0, np.arange(256), np.arange(256) + 1), 255)
    assert (first == want).all(), 'numpy.rint no longer rounds half to even?'
    np.savez_compressed(OUT, **out)
    print(OUT, f'{os.path.getsize(OUT) / 1e3:.0f} kB', {k: tuple(v.shape) for k, v in out.items() if not k.startswith('setup')})


if __name__ == '__main__':
    main()
