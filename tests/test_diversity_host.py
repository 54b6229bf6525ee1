"""Per-prompt diversity without a GPU: the pair order, the figures of a set, the grouping and refusals of tools/prompt_diversity.py, the
usage errors of generate_onestep.py --diversity (refused before a GPU is touched), and the two entry points in the C header."""
import importlib.util
import os

import numpy as np
import pytest

from sid_lsg_amd import diversity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LP = ['--lpips_vgg', 'random:lpips-vgg:1', '--lpips_lin', 'random:lpips-vgg:1']


def _tool():
    spec = importlib.util.spec_from_file_location('prompt_diversity', os.path.join(ROOT, 'tools', 'prompt_diversity.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pair_index_order_and_count():
    assert diversity.pair_index(2).tolist() == [[0, 1]]
    assert diversity.pair_index(3).tolist() == [[0, 1], [0, 2], [1, 2]]
    t = diversity.pair_index(16)
    assert tuple(t.shape) == (120, 2) and t[0].tolist() == [0, 1] and t[14].tolist() == [0, 15] and t[15].tolist() == [1, 2] and t[-1].tolist() == [14, 15]
    rows = t.tolist()
    assert rows == sorted(rows) and len(set(map(tuple, rows))) == 120 and all(i < j for i, j in rows)
    with pytest.raises(ValueError):
        diversity.pair_index(1)


def test_aggregate_on_hand_made_rows():
    rows = [dict(lpips=0.25, lpips_min=0.125, lpips_pairs=[0.125, 0.375], ssim=0.5, mse=4.0),
            dict(lpips=0.75, lpips_min=0.5, lpips_pairs=[0.5, 1.0], ssim=0.25, mse=8.0)]
    mean = diversity.aggregate(rows)
    assert mean == dict(groups=2, lpips=0.5, lpips_min=0.3125, ssim=0.375, mse=6.0, lpips_std=0.25)      # population std: sqrt((0.25^2 + 0.25^2) / 2)
    assert diversity.aggregate({'0': rows[0], '1': rows[1]}) == mean                                       # a dict keyed by group is read the same way
    one = diversity.aggregate(rows[:1])
    assert one['groups'] == 1 and one['lpips'] == 0.25 and one['lpips_std'] == 0.0
    with pytest.raises(ValueError):
        diversity.aggregate([])
    assert '2 groups' in diversity.format_means(mean) and 'lpips 0.5' in diversity.format_means(mean)


def test_groups_of_sample_keys():
    assert diversity.groups_of([0, 1, 2, 3, 4, 5], 3) == {0: [0, 1, 2], 1: [3, 4, 5]}
    assert diversity.groups_of([5, 4, 3, 8, 7, 6], 3) == {1: [3, 4, 5], 2: [6, 7, 8]}
    with pytest.raises(ValueError, match='whole groups of 3.*condition 0 has 2'):
        diversity.groups_of([1, 2, 3, 4, 5, 6], 3)
    diversity.check_group_size(2), diversity.check_group_size(16)
    for K in (1, 17):
        with pytest.raises(ValueError, match='2 .. 16'):
            diversity.check_group_size(K)


def _images(d, sizes):
    import PIL.Image
    os.makedirs(d, exist_ok=True)
    for i, (w, h) in enumerate(sizes):
        PIL.Image.fromarray(np.full((h, w, 3), 10 * i, np.uint8), 'RGB').save(os.path.join(d, f'{i:02d}.png'))
    return str(d)


def test_tool_grouping_and_refusals(tmp_path):
    from click.testing import CliRunner
    tool = _tool()
    files = [f'{i:02d}.png' for i in range(6)]
    assert tool.group_files(files, 3) == [files[:3], files[3:]] and tool.group_files(files, 2) == [files[:2], files[2:4], files[4:]]
    six = _images(tmp_path / 'six', [(16, 16)] * 6)
    five = _images(tmp_path / 'five', [(16, 16)] * 5)
    mixed = _images(tmp_path / 'mixed', [(16, 16), (16, 16), (16, 20), (16, 16)])
    small = _images(tmp_path / 'small', [(12, 16)] * 2)
    run = lambda *args: CliRunner().invoke(tool.main, list(args))  # noqa: E731
    r = run('--images', five, '--group', '3', *LP)
    assert r.exit_code == 2 and '5 PNG or JPEG files' in r.output and 'multiple of --group 3' in r.output
    r = run('--images', mixed, '--group', '2', *LP)
    assert r.exit_code == 2 and os.path.join(mixed, '02.png') in r.output and os.path.join(mixed, '00.png') in r.output and 'equal sizes' in r.output
    r = run('--images', six, '--group', '3')
    assert r.exit_code == 2 and '--lpips_vgg' in r.output and '--lpips_lin' in r.output
    r = run('--images', six, '--group', '3', '--lpips_vgg', 'random:lpips-vgg')
    assert r.exit_code == 2 and '--lpips_lin' in r.output
    r = run('--images', six, '--group', '3', '--lpips_vgg', 'random:lpips-vgg:1', '--lpips_lin', 'random:lpips-vgg:2')
    assert r.exit_code == 2 and 'one seed' in r.output
    r = run('--images', six, '--group', '1', *LP)
    assert r.exit_code == 2 and '--group' in r.output
    r = run('--images', six, '--group', '17', *LP)
    assert r.exit_code == 2 and '--group' in r.output
    r = run('--images', str(tmp_path / 'nowhere'), '--group', '2', *LP)
    assert r.exit_code == 2 and '--images' in r.output and 'not a directory' in r.output
    r = run('--images', small, '--group', '2', *LP)
    assert r.exit_code == 2 and '16 x 16' in r.output
    r = run('--images', six, '--group', '3', '--prompts', str(tmp_path / 'none.txt'), *LP)
    assert r.exit_code == 2 and '--prompts' in r.output and 'not a file' in r.output


def test_generate_usage_errors(tmp_path):
    from click.testing import CliRunner
    import generate_onestep as g
    run = lambda *a: CliRunner().invoke(g.main, ['--outdir', str(tmp_path / 'o'), '--repo_id', 'random:tiny', '--network', 'teacher', *a])  # noqa: E731
    r = run('--diversity', '1', *LP)
    assert r.exit_code == 2 and '--diversity' in r.output and '--seeds_per_prompt' in r.output
    r = run('--diversity', '1', '--seeds_per_prompt', '1', *LP)
    assert r.exit_code == 2 and '--seeds_per_prompt' in r.output
    r = run('--diversity', '1', '--seeds_per_prompt', '17', '--seeds', '0-16', *LP)
    assert r.exit_code == 2 and '--seeds_per_prompt 17' in r.output and '2 .. 16' in r.output
    r = run('--diversity', '1', '--seeds_per_prompt', '3', '--seeds', '0-5')
    assert r.exit_code == 2 and '--diversity' in r.output and '--lpips_vgg' in r.output and '--lpips_lin' in r.output
    r = run('--diversity', '1', '--seeds_per_prompt', '3', '--seeds', '0-5', '--lpips_vgg', 'random:lpips-vgg')
    assert r.exit_code == 2 and '--lpips_lin' in r.output
    r = run('--diversity', '1', '--seeds_per_prompt', '3', '--seeds', '0-6', *LP)
    assert r.exit_code == 2 and '7 samples' in r.output and 'multiple of --seeds_per_prompt 3' in r.output
    r = run('--diversity', '1', '--seeds_per_prompt', '3', '--seeds', '0-63', '--num', '4', *LP)           # --num cuts the list first
    assert r.exit_code == 2 and '4 samples' in r.output
    r = run('--diversity', '1', '--seeds_per_prompt', '3', '--seeds', '1-6', *LP)                           # a multiple of K, but no whole groups
    assert r.exit_code == 2 and 'whole groups of 3' in r.output
    r = run('--seeds_per_prompt', '0')
    assert r.exit_code == 2 and '--seeds_per_prompt' in r.output
    # the LPIPS specs without either consumer: refused, naming both
    r = run('--seeds_per_prompt', '3', *LP)
    assert r.exit_code == 2 and '--fidelity or --diversity' in r.output
    assert g.diversity_options(False, 1, None, None, [0, 1]) is None
    assert g.diversity_options(True, 2, LP[1], LP[3], [0, 1, 2, 3]) == (LP[1], LP[3], {0: [0, 1], 1: [2, 3]})
    assert g.fidelity_options(None, False, LP[1], LP[3], diversity=True) is None
    assert g.sample_path('out', False, 1234) == os.path.join('out', '001234.png') and g.sample_path('out', True, 1234) == os.path.join('out', '001000', '001234.png')
    assert not (tmp_path / 'o').exists()


def test_train_options_are_validated_by_name():
    import sid_train
    from sid_lsg_amd import metrics
    assert metrics.LPIPSDIV_METRICS == ('lpipsdiv1k_full', 'lpipsdiv_test') and all(metrics.is_valid_metric(m) for m in metrics.LPIPSDIV_METRICS)
    flags = [f for flags, _ in sid_train.OPTIONS for f in flags]
    assert '--metric_lpips_vgg' in flags and '--metric_lpips_lin' in flags
    opts = metrics.MetricOptions(G=None, prompts=['a'], device='cpu')
    assert opts.metric_lpips_vgg is None and opts.metric_lpips_lin is None and opts.lpips_detector is None
    with pytest.raises(ValueError, match='--metric_lpips_vgg.*--metric_lpips_lin'):
        metrics.compute_prompt_diversity(opts, 1, 4)


def test_header_declares_the_entry_points():
    from sid_lsg_amd._lib import parse_header
    import ctypes
    protos = parse_header()
    assert protos['sidlsg_lpips_group_ws_doubles'] == [ctypes.c_int] * 4
    p, i = ctypes.c_void_p, ctypes.c_int
    assert protos['sidlsg_lpips_group_f32'] == [p, i, p, i, i, i, i, i, p, p, p]


def test_fp64_preconditions_of_the_gpu_cases():
    """tests/test_gpu_diversity.py::test_group_layer_against_fp64 rests on these: two different pairs of a case are at least 4 bounds
    apart (so a value in another pair's slot is caught); the K = 16 cases are not, and are held to bit-equality only."""
    import diversity_cases as dc
    gaps = {case: dc.smallest_gap(case) for case in dc.FP64_CASES}
    print(gaps)
    assert all(g >= 4 for g in gaps.values()), gaps
    assert all(case in dc.BIT_CASES for case in dc.FP64_CASES) and len(dc.BIT_CASES) == 6
    assert dc.k_bound(64) == 26 and dc.k_bound(20) == 26 and dc.k_bound(128) == 34 and dc.k_bound(512) == 82
    assert dc.pair_table(3) == [(0, 1), (0, 2), (1, 2)]
