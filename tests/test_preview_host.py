"""Snapshot preview grids, host side (`-m "not gpu"`): the grid set-up against the reference's own setup_snapshot_image_grid
(tests/golden/preview_grid.npz, tools/make_preview_goldens.py), the chunking, the PNG writer, the argument checks of the grid kernel's
entry point and the command-line option."""
import inspect
import os
import struct
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Prompts:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return None, f'prompt {i}'


def _reference_split_list(lst, size):
    """What the reference's split_list returns for an integer size, by its description: full chunks, then the remainder."""
    sizes = [size] * (len(lst) // size) + ([len(lst) % size] if len(lst) % size else [])
    out, at = [], 0
    for s in sizes:
        out.append(lst[at:at + s])
        at += s
    return out


@pytest.mark.parametrize('n', [5, 1000])
@pytest.mark.parametrize('res', [256, 512, 768, 4096])
def test_grid_setup_matches_the_reference(golden_dir, res, n):
    from sid_lsg_amd import preview
    g = np.load(os.path.join(golden_dir, 'preview_grid.npz'))
    size, indices = preview.grid_layout(n, res)
    assert list(size) == g[f'setup_{res}_{n}_size'].tolist()
    assert indices == g[f'setup_{res}_{n}_indices'].tolist()
    grid = preview.setup_snapshot_grid(_Prompts(n), res, 8, (4, 2, 2), 'cpu')
    assert grid.size == size and grid.indices == indices
    assert [p for c in grid.c for p in c] == [f'prompt {i}' for i in indices]
    assert sum(len(z) for z in grid.z) == size[0] * size[1] and [len(z) for z in grid.z] == [len(c) for c in grid.c]


def test_grid_sizes_named_by_the_issue():
    from sid_lsg_amd import preview
    assert preview.grid_layout(10, 512)[0] == (7, 4) and preview.grid_layout(10, 768)[0] == (7, 4)
    assert preview.grid_layout(10, 256)[0] == (15, 8)


@pytest.mark.parametrize('batch_gpu', [1, 8, 28, 30])
def test_chunking_is_split_list(batch_gpu):
    from sid_lsg_amd import preview
    items = [f'p{i}' for i in range(28)]
    assert preview.split_chunks(items, batch_gpu) == _reference_split_list(items, batch_gpu)
    grid = preview.setup_snapshot_grid(_Prompts(40), 512, batch_gpu, (4, 2, 2), 'cpu')
    assert [len(c) for c in grid.c] == [len(c) for c in _reference_split_list(items, batch_gpu)]
    assert [len(z) for z in grid.z] == [len(c) for c in grid.c]


def test_grid_latents_come_from_a_private_generator():
    """grid_z is the seeded-2024 stream of its own generator; drawing it leaves the global generator where it was."""
    from sid_lsg_amd import preview
    torch.manual_seed(11)
    before = torch.random.get_rng_state()
    a = preview.setup_snapshot_grid(_Prompts(9), 512, 8, (4, 2, 2), 'cpu')
    assert torch.equal(torch.random.get_rng_state(), before)
    torch.manual_seed(12)
    b = preview.setup_snapshot_grid(_Prompts(9), 512, 28, (4, 2, 2), 'cpu')
    assert torch.equal(torch.cat(a.z), torch.cat(b.z))
    want = torch.randn([28, 4, 2, 2], generator=torch.Generator().manual_seed(2024))
    assert torch.equal(torch.cat(a.z), want)


def _decode_png(data):
    """RGB8, no interlace, filter 0 on every row, a single IDAT: what preview.png_bytes writes."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    w, h, depth, colour, _, _, interlace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, interlace) == (8, 2, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3)


def test_zlib_png_writer_round_trips_a_grid(golden_dir, tmp_path):
    from sid_lsg_amd import preview
    grid = np.load(os.path.join(golden_dir, 'preview_grid.npz'))['grid_m1_1']
    data = preview.png_bytes(grid)
    assert np.array_equal(_decode_png(data), grid)
    try:
        import PIL.Image
    except ImportError:
        PIL = None
    if PIL is not None:
        path = tmp_path / 'grid.png'
        path.write_bytes(data)
        assert np.array_equal(np.asarray(PIL.Image.open(path).convert('RGB')), grid)
    # save_png (either writer) round-trips too; generate_onestep.py uses the same function
    import generate_onestep
    assert generate_onestep.save_png is preview.save_png
    preview.save_png(str(tmp_path / 'saved.png'), grid)
    saved = (tmp_path / 'saved.png').read_bytes()
    back = np.asarray(PIL.Image.open(tmp_path / 'saved.png').convert('RGB')) if PIL is not None else _decode_png(saved)
    assert np.array_equal(back, grid)


def test_grid_kernel_entry_point_rejects_bad_arguments_without_launching():
    """The EINVAL cases are host-side argument checks: they return before anything is launched, so they run without a GPU."""
    from sid_lsg_amd._lib import lib
    lib.load()
    src = torch.zeros(4 * 3 * 16 * 16 + 8, dtype=torch.float32)
    grid = torch.full((4 * 16 * 7 * 16 * 3,), 7, dtype=torch.uint8)
    fn = lib.sidlsg_image_grid_u8.raw
    sp, gp = src.data_ptr(), grid.data_ptr()
    assert sp % 16 == 0
    #          src grid  B   H   W  layout first gw gh  lo   hi
    bad = [(sp, gp, 4, 16, 16, 1, 25, 7, 4, -1.0, 1.0),        # first + B > gw * gh
           (sp, gp, 29, 16, 16, 1, 0, 7, 4, -1.0, 1.0),
           (sp, gp, 4, 16, 16, 1, 0, 7, 4, 1.0, 1.0),           # hi == lo
           (None, gp, 4, 16, 16, 1, 0, 7, 4, -1.0, 1.0),        # null pointers
           (sp, None, 4, 16, 16, 1, 0, 7, 4, -1.0, 1.0),
           (sp, gp, 1, 1024, 1024, 1, 0, 32, 32, -1.0, 1.0),    # 32768 x 32768 x 3 bytes >= 2 GiB
           (sp, gp, 1, 16384, 16384, 0, 0, 7, 4, -1.0, 1.0),
           (sp, gp, 4, 16, 18, 1, 0, 7, 4, -1.0, 1.0),          # W % 4
           (sp, gp, 4, 16, 16, 2, 0, 7, 4, -1.0, 1.0),          # unknown layout
           (sp, gp, 4, 16, 16, 1, -1, 7, 4, -1.0, 1.0),
           (sp + 4, gp, 4, 16, 16, 1, 0, 7, 4, -1.0, 1.0)]      # source not 16-byte aligned
    for args in bad:
        assert fn(*args, None) == -22, args
    assert bool((grid == 7).all())


def test_cli_option_reaches_the_training_loop(tmp_path, golden_dir, monkeypatch):
    from click.testing import CliRunner
    import sid_train
    from sid_lsg_amd.training_loop import evaluate_network, training_loop
    assert inspect.signature(training_loop).parameters['snapshot_images'].default is False
    assert inspect.signature(evaluate_network).parameters['snapshot_images'].default is False
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a red cube\na blue sphere\n')
    monkeypatch.chdir(tmp_path)
    base = ['--outdir', 'runs', '--data_prompt_text', '.', '--sd_model', 'random:tiny', '--seed', '3', '--batch', '8', '--batch-gpu', '2',
            '--duration', '0.01', '--ema', '0.05', '--cfg_train_fake', '1.5', '--cfg_eval_fake', '1.5', '--cfg_eval_real', '1.5', '--dry-run']
    outputs = {}
    for extra, want in (((), False), (('--snapshot_images', '1'), True), (('--snapshot_images', '0'), False)):
        seen = {}
        orig = sid_train.build_config

        def spy(o):
            seen['c'] = orig(o)
            return seen['c']
        monkeypatch.setattr(sid_train, 'build_config', spy)
        res = CliRunner().invoke(sid_train.main, base + list(extra))
        monkeypatch.setattr(sid_train, 'build_config', orig)
        assert res.exit_code == 0, res.output
        assert bool(seen['c'].get('snapshot_images', False)) is want
        inspect.signature(training_loop).bind(**seen['c'])                 # every key is a keyword of the loop
        outputs[extra] = res.output
    # without the option the dry run prints what it printed before the option existed
    with open(os.path.join(golden_dir, 'sid_train_dry_run.txt')) as f:
        assert outputs[()] == f.read()
    assert outputs[('--snapshot_images', '0')] == outputs[()]
    assert '"snapshot_images": true' in outputs[('--snapshot_images', '1')]
