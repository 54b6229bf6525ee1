"""Host side of the Canny / edge-adherence feature: the restatement of tests/canny_ref.py on hand-made cases whose answer can be read
off the rule, the host rules of sid_lsg_amd.edges (adherence_rows, aggregate, the bit-plane helpers), every usage error of the command
lines and tools by name, and the C ABI's declarations.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

import canny_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


# ---- the restatement on cases with a known answer ----
def test_a_vertical_step_gives_one_column_and_the_plateau_rule_names_it():
    """Columns 0..3 at 0, 4..7 at 200: |dx| = 800 on columns 3 and 4 (a two-pixel plateau), 0 elsewhere.  The horizontal rule is
    m > left && m >= right: column 3 has left 0 and right 800 -> kept; column 4 has left 800 -> dropped."""
    cand, strong, m = cr.classify_ref(cr.step_edge(), 100, 200)
    assert (m[:, 3] == 800).all() and (m[:, 4] == 800).all() and not m[:, [0, 1, 2, 5, 6, 7]].any()
    want = np.zeros((8, 8), dtype=bool)
    want[:, 3] = True
    assert np.array_equal(cand, want) and np.array_equal(strong, want)
    assert np.array_equal(cr.canny_ref(cr.step_edge()), want)


def test_the_mirrored_step_keeps_the_left_pixel_of_its_plateau_too():
    """The rule looks at positions, not at the sign of the gradient: the falling step keeps column 3 as well."""
    img = cr.step_edge()[:, ::-1].copy()              # 200 on columns 0..3
    cand, _, m = cr.classify_ref(img)
    assert (m[:, 3] == 800).all() and (m[:, 4] == 800).all()
    assert cand[:, 3].all() and not cand[:, 4].any()


def test_an_edge_in_channel_b_alone_is_found():
    """Rows 4..7 at 220 in B only: |dy| = 880 on rows 3 and 4; the vertical rule m > above && m >= below keeps row 3."""
    cand, strong, m = cr.classify_ref(cr.blue_only_edge())
    assert (m[3] == 880).all() and (m[4] == 880).all()
    assert cand[3].all() and strong[3].all() and cand.sum() == 8


def test_the_first_channel_wins_a_tie():
    """R has a vertical step, G a horizontal one of the same height; where both give the same magnitude R's (dx, dy) is taken."""
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    img[:, 4:, 0] = 100
    img[4:, :, 1] = 100
    dx, dy, m = cr.sobel_ref(img)
    assert m[1, 3] == 400 and dx[1, 3] == 400 and dy[1, 3] == 0          # only R has a gradient here
    assert m[3, 1] == 400 and dx[3, 1] == 0 and dy[3, 1] == 400          # only G
    assert m[3, 3] == 400 and (dx[3, 3], dy[3, 3]) == (400, 0)           # R: (400, 0), G: (0, 400) -- a tie, R's pair
    assert cr.sobel_ref(img[:, :, [1, 0, 2]])[1][3, 3] == 400             # with the channels swapped the other pair is taken


def test_thresholds_are_strict():
    img = cr.step_edge()                               # every non-zero magnitude is 800
    assert cr.classify_ref(img, 799, 799)[0].sum() == 8 and cr.classify_ref(img, 799, 799)[1].sum() == 8
    assert cr.classify_ref(img, 800, 800)[0].sum() == 0                  # m == low is not a candidate
    cand, strong, _ = cr.classify_ref(img, 100, 800)
    assert cand.sum() == 8 and strong.sum() == 0                         # m == high is not strong
    assert cr.canny_ref(img, 100, 800).sum() == 0                        # and without a strong pixel nothing is an edge


def test_the_magnitude_outside_the_image_is_zero():
    """A step between columns 0 and 1: column 0's left neighbour is outside the image (0), so it survives the > test."""
    cand, _, m = cr.classify_ref(cr.step_edge(x0=1))
    assert (m[:, 0] == 800).all() and cand[:, 0].all() and not cand[:, 1].any()


def test_hysteresis_keeps_components_with_a_strong_pixel():
    cand = np.zeros((5, 9), dtype=bool)
    cand[1, 0:3] = True                                # component A, diagonal link to (2, 3)
    cand[2, 3] = True
    cand[4, 6:9] = True                                # component B, no strong pixel
    strong = np.zeros_like(cand)
    strong[1, 0] = True
    strong[0, 8] = True                                # strong outside cand: ignored
    want = cand.copy()
    want[4] = False
    assert np.array_equal(cr.hysteresis_ref(cand, strong), want)


def test_the_recipes_of_the_gpu_tests_are_not_trivial():
    for (H, W, sigma, seed), counts in (((64, 64, 2.0, 2), (1207, 777, 315, 115)), ((40, 136, 2.5, 3), (1370, 474, 607, 289))):
        cand, strong, _ = cr.classify_ref(cr.smoothed_noise(H, W, sigma, seed))
        e = cr.hysteresis_ref(cand, strong)
        assert (int(cand.sum()), int(strong.sum()), int((e & ~strong).sum()), int((cand & ~e).sum())) == counts
    cand, strong = cr.serpentine(64)
    assert cr.geodesic_depth(cand, strong) > 2000 and np.array_equal(cr.hysteresis_ref(cand, strong), cand)


def test_match_ref_counts():
    a = np.zeros((4, 6), dtype=bool)
    b = np.zeros((4, 6), dtype=bool)
    a[0, 0] = a[3, 5] = True
    b[1, 1] = b[3, 2] = True
    assert cr.match_ref(a, b, 0) == [2, 2, 0, 0]
    assert cr.match_ref(a, b, 1) == [2, 2, 1, 1]
    assert cr.match_ref(a, b, 3) == [2, 2, 2, 2]


# ---- sid_lsg_amd.edges: host rules ----
def test_bit_plane_helpers_round_trip():
    from sid_lsg_amd import edges
    rng = np.random.default_rng(0)
    for W in (1, 31, 32, 33, 72):
        m = rng.random((2, 3, W)) < 0.5
        words = edges.pack_bits(m)
        assert words.dtype == np.int32 and words.shape == (2, 3, (W + 31) // 32)
        assert np.array_equal(edges.unpack_bits(words, W), m)
        if W % 32:
            assert not (words[..., -1].view(np.uint32) >> (W % 32)).any()
    assert edges.pack_bits(np.array([True] + [False] * 30 + [True])).view(np.uint32).tolist() == [0x80000001]


def test_adherence_rows():
    from sid_lsg_amd import edges
    rows = edges.adherence_rows([[10, 20, 5, 8], [0, 4, 0, 0], [3, 0, 0, 0], [5, 5, 0, 0], [0, 0, 0, 0]])
    r = rows[0]          # counts are |control|, |output|, control hits, output hits
    assert (r['control_edges'], r['output_edges'], r['control_hits'], r['output_hits']) == (10, 20, 5, 8)
    assert r['precision'] == 8 / 20 and r['recall'] == 5 / 10 and r['f1'] == pytest.approx(2 * 0.4 * 0.5 / 0.9, rel=1e-15)
    assert math.isnan(rows[1]['recall']) and rows[1]['precision'] == 0 and math.isnan(rows[1]['f1'])
    assert math.isnan(rows[2]['precision']) and rows[2]['recall'] == 0 and math.isnan(rows[2]['f1'])
    assert rows[3]['precision'] == 0 and rows[3]['recall'] == 0 and rows[3]['f1'] == 0
    assert all(math.isnan(rows[4][k]) for k in ('precision', 'recall', 'f1'))


def test_aggregate_is_micro_averaged():
    from sid_lsg_amd import edges
    rows = edges.adherence_rows([[10, 20, 5, 8], [0, 4, 0, 0], [1000, 1000, 900, 800]])
    mean = edges.aggregate({f'{i}.png': r for i, r in enumerate(rows)})
    assert (mean['control_edges'], mean['output_edges'], mean['control_hits'], mean['output_hits']) == (1010, 1024, 905, 808)
    assert mean['precision'] == 808 / 1024 and mean['recall'] == 905 / 1010
    p, r = 808 / 1024, 905 / 1010
    assert mean['f1'] == 2 * p * r / (p + r)
    assert mean['images'] == 3
    assert mean['f1_macro'] == (rows[0]['f1'] + rows[2]['f1']) / 2               # the image whose f1 is NaN is left out
    assert edges.aggregate(rows) == mean
    empty = edges.aggregate(edges.adherence_rows([[0, 0, 0, 0]]))
    assert all(math.isnan(empty[k]) for k in ('precision', 'recall', 'f1', 'f1_macro')) and empty['images'] == 1
    with pytest.raises(ValueError, match='no images'):
        edges.aggregate([])


def test_python_refusals_name_the_argument():
    import torch
    from sid_lsg_amd import edges
    with pytest.raises(ValueError, match='low = 300 is above high = 200'):
        edges.check_thresholds(300, 200)
    with pytest.raises(ValueError, match='low = -1'):
        edges.check_thresholds(-1, 200)
    with pytest.raises(ValueError, match='high = -5'):
        edges.check_thresholds(0, -5)
    for r in (-1, 17, 1.5):
        with pytest.raises(ValueError, match='tolerance'):
            edges.check_tolerance(r)
    with pytest.raises(ValueError, match=r'1024 x 1024.*262144 bytes.*147456'):
        edges.check_size(1024, 1024)
    edges.check_size(768, 768)
    with pytest.raises(ValueError, match=r'canny: images: expected uint8 \[B, H, W, 3\]'):
        edges.canny(torch.zeros(2, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match='pack: threshold'):
        edges.pack(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 256)


# ---- the C ABI ----
def test_the_entry_points_are_declared():
    from sid_lsg_amd._lib import parse_header
    protos = parse_header()
    for name, nargs in (('sidlsg_canny_classify_u8', 9), ('sidlsg_edge_hysteresis', 9), ('sidlsg_edge_pack_u8', 7), ('sidlsg_edge_match_counts', 8)):
        assert name in protos and len(protos[name]) == nargs, name
    from sid_lsg_amd.csrc import build
    assert 'canny.hip' in build.SOURCES and 'canny.hip' not in build.EXTRA


# ---- usage errors, before a GPU is touched ----
def _dirs(tmp_path, size=(24, 24)):
    import PIL.Image
    ctl, prompts = tmp_path / 'ctl', tmp_path / 'prompts.txt'
    ctl.mkdir()
    PIL.Image.fromarray(np.zeros(size + (3,), dtype=np.uint8)).save(str(ctl / 'a.png'))
    prompts.write_text('a cube\n')
    return ctl, prompts


def _usage(main, args, text):
    from click.testing import CliRunner
    res = CliRunner().invoke(main, [str(a) for a in args])
    assert res.exit_code == 2, res.output
    assert text in res.output, res.output


def test_generate_onestep_usage_errors(tmp_path, monkeypatch):
    import generate_onestep as g
    import torch
    monkeypatch.setattr(g.dist, 'init', lambda: pytest.fail('a usage error must be raised before the process group is set up'))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    ctl, prompts = _dirs(tmp_path)
    base = ['--network', 'teacher', '--repo_id', 'random:tiny', '--outdir', tmp_path / 'out', '--text_prompts', prompts, '--resolution', 64]
    net = ['--controlnet', 'random:controlnet', '--control_images', ctl]
    for opts, flag in ((['--control_preprocess', 'canny'], '--control_preprocess'), (['--canny_low', 50], '--canny_low'), (['--canny_high', 50], '--canny_high'),
                       (['--control_adherence', 1], '--control_adherence'), (['--edge_tolerance', 2], '--edge_tolerance')):
        _usage(g.main, base + opts, f'{flag} apply to --controlnet only')
    _usage(g.main, base + net + ['--canny_low', 50], '--canny_low: the Canny thresholds and the tolerance apply to --control_preprocess canny or --control_adherence 1')
    _usage(g.main, base + net + ['--canny_high', 50], '--canny_high: the Canny thresholds')
    _usage(g.main, base + net + ['--control_preprocess', 'canny', '--edge_tolerance', 2], '--edge_tolerance applies to --control_adherence 1 only')
    pre = base + net + ['--control_preprocess', 'canny']
    _usage(g.main, pre + ['--canny_low', 201], '--canny_low 201 is above --canny_high 200')
    _usage(g.main, pre + ['--canny_low', 60, '--canny_high', 50], '--canny_low 60 is above --canny_high 50')
    _usage(g.main, pre + ['--canny_low', -1], '--canny_low -1: cannot be negative')
    _usage(g.main, pre + ['--canny_high', -1], '--canny_high -1: cannot be negative')
    adh = base + net + ['--control_adherence', 1]
    _usage(g.main, adh + ['--edge_tolerance', -1], '--edge_tolerance -1: cannot be negative')
    _usage(g.main, adh + ['--edge_tolerance', 17], '--edge_tolerance 17: at most 16 pixels')
    big = [str(a) for a in adh]
    big[big.index('--resolution') + 1] = '1024'
    _usage(g.main, big, '--resolution 1024: the Canny hysteresis keeps both bit planes of an image on chip, 262144 bytes here against a limit of 147456')
    _usage(g.main, base + net + ['--control_preprocess', 'sobel'], "'sobel' is not")


def test_tool_usage_errors(tmp_path, monkeypatch):
    import PIL.Image
    import torch
    import canny_edges
    import edge_adherence
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    ctl, _ = _dirs(tmp_path)
    out = tmp_path / 'out'
    _usage(canny_edges.main, ['--images', tmp_path / 'none', '--out', out, '--resolution', 64], 'not a directory')
    (tmp_path / 'empty').mkdir()
    _usage(canny_edges.main, ['--images', tmp_path / 'empty', '--out', out, '--resolution', 64], 'no PNG or JPEG files')
    _usage(canny_edges.main, ['--images', ctl, '--out', out, '--resolution', 64, '--canny_low', 300], '--canny_low 300 is above --canny_high 200')
    _usage(canny_edges.main, ['--images', ctl, '--out', out, '--resolution', 64, '--canny_low', -2], '--canny_low -2: cannot be negative')
    _usage(canny_edges.main, ['--images', ctl, '--out', out, '--resolution', 64, '--canny_high', -2], '--canny_high -2: cannot be negative')
    _usage(canny_edges.main, ['--images', ctl, '--out', out, '--resolution', 1024], '--resolution 1024: the Canny hysteresis')
    _usage(canny_edges.main, ['--images', ctl, '--out', out], "Missing option '--resolution'")
    assert not out.exists()
    imgs = tmp_path / 'imgs'
    imgs.mkdir()
    PIL.Image.fromarray(np.zeros((24, 32, 3), dtype=np.uint8)).save(str(imgs / 'x.png'))
    _usage(edge_adherence.main, ['--control', ctl, '--images', imgs], 'x.png is 32 x 24 but its control image')
    _usage(edge_adherence.main, ['--control', ctl, '--images', tmp_path / 'none'], '--images')
    _usage(edge_adherence.main, ['--control', tmp_path / 'empty', '--images', imgs], '--control')
    _usage(edge_adherence.main, ['--control', ctl, '--images', ctl, '--edge_tolerance', 17], '--edge_tolerance 17: at most 16 pixels')
    _usage(edge_adherence.main, ['--control', ctl, '--images', ctl, '--edge_tolerance', -1], '--edge_tolerance -1: cannot be negative')
    _usage(edge_adherence.main, ['--control', ctl, '--images', ctl, '--canny_low', 201], '--canny_low 201 is above --canny_high 200')
    _usage(edge_adherence.main, ['--control', ctl, '--images', ctl, '--canny_high', -3], '--canny_high -3: cannot be negative')
    big = tmp_path / 'big'
    big.mkdir()
    PIL.Image.fromarray(np.zeros((1024, 1024, 3), dtype=np.uint8)).save(str(big / 'b.png'))
    _usage(edge_adherence.main, ['--control', big, '--images', big], 'b.png is 1024 x 1024: the Canny hysteresis')
