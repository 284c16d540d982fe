"""CPU: the restatement of the 2D result video (tests/vis2d_restate.py) against the reference's own recorded output
(tests/golden/vis2d_T24.npz, tools/gen_golden_vis2d.py), the embedded colour tables, the track panel's rasterisation rules and the
PNG writer of l4p_amd/utils/vis2d.py."""
import json
import os

import numpy as np
import pytest

from l4p_amd.utils import vis2d as V
from tests import vis2d_restate as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vis2d_T24")
F = np.float32
SCENE_KEYS = ("rgb_u8", "depth_q", "flow_q", "mask_q", "traj_q", "vis_q", "key_y")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD + ".npz")
    g = {k: z[k] for k in z.files}
    return g, json.load(open(GOLD + ".json")), {k: g[k] for k in SCENE_KEYS}


def test_scene_is_the_fixtures_and_keeps_its_margins(gold):
    g, prov, sc = gold
    fresh = RS.make_scene()
    for k in SCENE_KEYS:
        assert np.array_equal(fresh[k], sc[k]), k
    _, T, H, W = sc["rgb_u8"].shape
    assert (T, H, W, sc["traj_q"].shape[0]) == (prov["T"], prov["H"], prov["W"], prov["N"]) and T > RS.TRACKS_LEAVE_TRACE + 1
    assert np.abs(sc["mask_q"] / 16.0 - np.log(0.85 / 0.15)).min() > 1e-3 and np.abs(sc["vis_q"] / 256.0).min() > 1e-3
    mag = np.hypot(*(sc["flow_q"] / 8.0))
    assert mag.min() < 1 and mag.max() > 25 and (mag < 25).mean() > 0.2
    depth = (sc["depth_q"].astype(np.float64) - 8) / 32
    assert (depth <= 0).any() and 0 < depth[depth > 0].min() < 0.05
    assert len(set(sc["key_y"].tolist())) == len(sc["key_y"])  # distinct start heights: the reference's argsort has no ties
    x = sc["traj_q"][3, 0] / 4.0
    assert x[0] < W and x[-1] > W + 2  # one track leaves the image
    assert (sc["vis_q"][5, 4:9] < 0).all()  # one has an invisible stretch


def test_dense_panels_equal_the_reference(gold):
    g, prov, sc = gold
    batch, out = RS.scene_tensors(sc)
    d = RS.restate_dense(batch, out, RS.TASKS)
    keep = prov["keep_frames"]
    assert np.array_equal(d["rgb"][keep], g["rgb_keep"])
    assert np.array_equal(d["grey"][keep], g["grey_keep"])
    assert np.array_equal(d["depth_index"], g["depth_index"])
    assert np.array_equal(d["flow_level"], g["flow_level"])
    assert np.array_equal(np.packbits(d["mask_bit"]), g["mask_bit"])
    assert d["depth_range"][0] == 0.05 and d["depth_range"][1] == (int(sc["depth_q"].max()) - 8) / 32 and d["flow_rad_max"] == 25.0


def test_call_sequence_equals_the_reference(gold):
    g, prov, sc = gold
    batch, out = RS.scene_tensors(sc)
    order, xy, vis, colors = RS.display_list(batch, out)
    assert np.array_equal(order, np.argsort(sc["key_y"], kind="stable"))
    kind, pts, col, wts = RS.expand_calls(xy, vis, colors)
    assert len(kind) == prov["calls"] and {RS.LINE, RS.BLEND, RS.CIRCLE} == set(kind.tolist())
    assert np.array_equal(kind, g["call_kind"])
    assert np.array_equal(pts, g["call_points"])
    assert np.array_equal(wts, g["call_weights"])
    # the colours: the reference hands cv2 float64 triples, the engine holds them in f32 - one rounding
    assert np.abs(col.astype(F).astype(np.float64) - g["call_colour"]).max() <= 2.0 ** -24 * np.abs(g["call_colour"]).max()
    assert np.array_equal(col, g["call_colour"])  # (and the restatement's own float64 colours are the reference's)


def test_embedded_tables():
    import matplotlib

    assert np.array_equal(V.turbo_table(), matplotlib.colormaps["turbo"](np.linspace(0, 1, 256))[:, :3])
    # the wheel by its definition (Baker et al. 2007): six hue segments of 15, 6, 4, 11, 13, 6 entries, one channel ramping
    want, col = np.zeros((55, 3)), 0
    for n, fixed, ramp, up in ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True), (6, 0, 2, False)):
        r = np.floor(255 * np.arange(n) / n)
        want[col:col + n, fixed] = 255
        want[col:col + n, ramp] = r if up else 255 - r
        col += n
    assert np.array_equal(V.colorwheel(), want)


def _blank(h=12, w=14):
    return np.full((h, w, 3), 0.25, F)


RED = np.array([1.0, 0.0, 0.5], F)
BLUE = np.array([0.0, 0.25, 1.0], F)


def _painted(img):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero((img != F(0.25)).any(-1)))}


def test_axis_aligned_and_zero_length_segments_paint_exactly_their_pixels():
    img = _blank()
    RS.raster_segment(img, 3, 5, 9, 5, RED)
    assert _painted(img) == {(x, 5) for x in range(3, 10)} and all((img[5, x] == RED).all() for x in range(3, 10))
    img = _blank()
    RS.raster_segment(img, 4, 8, 4, 2, RED)
    assert _painted(img) == {(4, y) for y in range(2, 9)} and all((img[y, 4] == RED).all() for y in range(2, 9))
    img = _blank()
    RS.raster_segment(img, 6, 6, 6, 6, RED)
    assert _painted(img) == {(6, 6)} and (img[6, 6] == RED).all()
    img = _blank()  # a diagonal: its own pixels fully, the neighbours at distance 1 / sqrt 2 partly
    RS.raster_segment(img, 2, 2, 6, 6, RED)
    assert all((img[k, k] == RED).all() for k in range(2, 7))
    c = F(1) - np.sqrt(F(0.5))
    assert np.array_equal(img[3, 4], (F(1) - c) * F(0.25) + c * RED)


def test_disc_pattern_and_clipping():
    img = _blank()
    RS.raster_disc(img, 6, 5, RED)
    rows = {}
    for x, y in _painted(img):
        rows.setdefault(y, []).append(x)
    assert [len(rows[y]) for y in sorted(rows)] == [3, 5, 5, 5, 3] and sorted(rows) == [3, 4, 5, 6, 7]
    img = _blank()
    RS.raster_disc(img, 0, 0, RED)  # clipped at the corner: rows of 3, 3, 2
    assert _painted(img) == {(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (0, 2), (1, 2)}
    RS.raster_disc(img, -5, 30, RED)  # wholly outside
    RS.raster_segment(img, -9, 3, -3, 3, BLUE)
    assert len(_painted(img)) == 8
    img = _blank()
    RS.raster_segment(img, 10, 4, 30, 4, RED)  # clipped at the right border
    assert _painted(img) == {(x, 4) for x in range(10, 14)}


def _list(points, vis=None):
    """display list of len(points) frames x tracks from points[t][i] = (x, y)"""
    xy = np.array(points, np.int64)
    return xy, np.ones(xy.shape[:2], bool) if vis is None else np.array(vis, bool)


def test_frame_ordering_fades_and_end_points():
    grey = np.full((12, 14), 0.25, F)
    cols = np.stack([RED, BLUE]).astype(np.float64)
    # two tracks crossing at (5, 5): the later rank overwrites the earlier one
    xy, vis = _list([[(2, 5), (5, 2)], [(8, 5), (5, 8)], [(8, 5), (5, 8)]])
    f1 = RS.raster_frame(grey, 1, xy, vis, cols)
    assert (f1[5, 5] == BLUE).all() and (f1[5, 3] == RED).all() and (f1[3, 5] == BLUE).all()  # one step, alpha = 1
    assert (f1[5, 8] == RED).all() and (f1[6, 9] == RED).all() and (f1[2, 8] != RED).any()  # the disc at the end point
    f0 = RS.raster_frame(grey, 0, xy, vis, cols)  # t = 0: discs only
    assert _painted(f0) == {(2 + dx, 5 + dy) for dx in range(-2, 3) for dy in range(-2, 3) if dx * dx + dy * dy <= 5} | \
        {(5 + dx, 2 + dy) for dx in range(-2, 3) for dy in range(-2, 3) if dx * dx + dy * dy <= 5}
    # fades: over L = 4 points the segment of step 0 is fainter than that of the last step
    xy, vis = _list([[(1, 1)], [(1, 10)], [(12, 10)], [(12, 1)]])
    f3 = RS.raster_frame(grey, 3, xy, vis, cols[:1])
    first, last = f3[5, 1], f3[10, 6]  # on step 0's and step 1's segments; step 2's is at full strength
    assert (f3[5, 12] == RED).all()
    assert abs(first[0] - 1) > abs(last[0] - 1) > 0 and abs(first[0] - 0.25) > 0
    w = [(F((s + 1) / 3), F(1 - (s + 1) / 3)) for s in range(3)]
    want = w[0][0] * RED + w[0][1] * F(0.25)  # painted at step 0, then carried through two more blends with itself as the start
    for a, b in w[1:]:
        want = a * want + b * want
    assert np.array_equal(first, want)
    # an invisible end point removes both its segments and its disc
    xy, vis = _list([[(1, 1)], [(1, 10)], [(12, 10)]], vis=[[1], [0], [1]])
    f2 = RS.raster_frame(grey, 2, xy, vis, cols[:1])
    assert _painted(f2) == {(12 + dx, 10 + dy) for dx in range(-2, 2) for dy in range(-2, 2) if dx * dx + dy * dy <= 5}


def test_restated_video_layout_and_task_subsets(gold):
    _, _, sc = gold
    batch, out = RS.scene_tensors(sc)
    full = RS.restate(batch, out, RS.TASKS, track_frames=(0, 20))
    _, T, H, W = sc["rgb_u8"].shape
    assert full["video"].shape == (T, H, 5 * W, 3) and full["video"].dtype == F
    sub = RS.restate(batch, out, ["dyn_mask", "camray", "depth"], track_frames=())
    assert sub["video"].shape == (T, H, 3 * W, 3)
    assert np.array_equal(sub["video"][:, :, W:2 * W], full["video"][:, :, 3 * W:4 * W])
    assert np.array_equal(sub["video"][:, :, 2 * W:], full["video"][:, :, W:2 * W])
    tr = full["video"][:, :, 4 * W:]
    assert (tr[5, ..., 0] == tr[5, ..., 1]).all() and (tr[20, ..., 0] != tr[20, ..., 1]).any()
    with pytest.raises(ValueError):
        V.panel_slots(["depth", "depth"])


def test_png_writer_round_trips_uint8_frames(tmp_path):
    g = np.random.default_rng(3)
    vid = g.random((3, 10, 22, 3)).astype(F)
    vid[0, 0, :4, 0] = [-0.5, 0.0, 1.0, 1.5]
    u8 = V.to_uint8(vid)
    assert u8.dtype == np.uint8 and u8[0, 0, :4, 0].tolist() == [0, 0, 255, 255]
    assert np.array_equal(u8, np.floor(np.clip(vid.astype(F) * F(255) + F(0.5), 0, 255)).astype(np.uint8))
    name = V.write_video(vid, str(tmp_path / "o"), "clip")
    try:
        import mediapy  # noqa: F401
    except ImportError:
        assert name == str(tmp_path / "o" / "clip") and sorted(os.listdir(name)) == ["00000.png", "00001.png", "00002.png"]
        assert np.array_equal(V.read_png_frames(name), u8)
    d = V.write_png_frames(u8, str(tmp_path / "p"))
    assert np.array_equal(V.read_png_frames(d), u8)
