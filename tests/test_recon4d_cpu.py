"""CPU: the 4D reconstruction's yardsticks (l4p_amd/utils/recon4d.py).

* tests/recon4d_restate.py (plain torch) reproduces the reference's own generate_4D_visualization output recorded in
  tests/golden/recon4d_T24.npz (tools/gen_golden_recon4d.py): counts and scale exact, points within 1e-6 of the scene extent;
* the hsv table / index rule equal matplotlib's for every track count 1..2048;
* PLY write / read round trip; file names and dict keys of the return value equal the reference's."""
import json
import os

import numpy as np
import pytest
import torch

from l4p_amd.utils import recon4d as R
from tests import recon4d_restate as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "recon4d_T24")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD + ".npz")
    return {k: z[k] for k in z.files}, json.load(open(GOLD + ".json"))


def _scene(g):
    return {k: g[k] for k in ("rgb_u8", "depth_q", "poses", "K", "traj", "vis_logit", "track_depth")}


def _frame(res, t, hw, tracks):
    pts, col = res["points"][t * hw:(t + 1) * hw], res["colors"][t * hw:(t + 1) * hw]
    if tracks:
        a, b = res["track_offsets"][t], res["track_offsets"][t + 1]
        pts, col = np.concatenate([pts, res["track_xyz"][a:b]]), np.concatenate([col, res["track_colors"][a:b]])
    return pts, col


@pytest.mark.parametrize("tracks", [True, False])
def test_restatement_reproduces_the_reference(gold, tracks):
    g, prov = gold
    batch, out = RS.scene_tensors(_scene(g))
    tasks = ["depth", "camray"] + (["track_2d"] if tracks else [])
    res = RS.restate(batch, out, tasks)
    T, H, W = g["depth_q"].shape
    tag = "track" if tracks else "plain"
    counts = np.array([_frame(res, t, H * W, tracks)[0].shape[0] for t in range(T)])
    assert np.array_equal(counts, g[f"{tag}_count"])
    ext = RS.extent(g[f"{tag}_xyz_0"])
    for t in prov["keep_frames"]:
        pts, col = _frame(res, t, H * W, tracks)
        err = np.abs(pts.astype(np.float64) - g[f"{tag}_xyz_{t}"]).max() / ext
        assert err <= 1e-6, (t, err)
        assert np.array_equal(col, g[f"{tag}_rgb_{t}"]), t
    fr = np.asarray(g[f"{tag}_frustum"])
    assert np.abs(res["frustum"] - fr).max() <= 1e-6 * RS.extent(fr)
    if tracks:
        assert res["scale"].view(np.int32)[0] == g["scale"].view(np.int32)[0]
        assert np.array_equal(res["track_counts"], g["vis_count"])
    # the frustum's normals, triangles and colour as the reference's mesh carries them
    assert np.abs(R.frustum_normals() - g[f"{tag}_frustum_normals"]).max() <= 1e-7
    assert np.array_equal(R.FRUSTUM_TRIANGLES, g[f"{tag}_frustum_triangles"])
    assert np.array_equal(R.colour_bytes(R.FRUSTUM_COLOUR), R.colour_bytes(g[f"{tag}_frustum_colour"]))


def test_hsv_table_and_index_equal_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    import matplotlib.colors as mc

    cmap = matplotlib.colormaps["hsv"]
    table = R.hsv_table()
    assert np.array_equal(table, cmap(np.arange(256))[:, :3])
    lut = R.colour_bytes(table)
    for n in range(1, 2049):
        norm = mc.Normalize(vmin=0, vmax=n - 1)
        i = np.arange(n)
        want = R.colour_bytes(np.array([cmap(norm(k))[:3] for k in i]) if n <= 64 else cmap(norm(i))[:, :3])
        assert np.array_equal(lut[R.hsv_index(i, n)], want), n


def test_ply_round_trip(tmp_path):
    g = np.random.default_rng(1)
    xyz = g.normal(size=(37, 3)).astype(np.float32)
    rgb = g.integers(0, 256, size=(37, 3), dtype=np.uint8)
    R.write_ply(str(tmp_path / "a.ply"), xyz, rgb)
    back = R.read_ply(str(tmp_path / "a.ply"))
    assert set(back) == {"xyz", "rgb"} and np.array_equal(back["xyz"], xyz) and np.array_equal(back["rgb"], rgb)
    v = R.frustum_camera_vertices().astype(np.float32)
    R.write_ply(str(tmp_path / "m.ply"), v, np.full((8, 3), 7, np.uint8), normals=R.frustum_normals(), faces=R.FRUSTUM_TRIANGLES)
    m = R.read_ply(str(tmp_path / "m.ply"))
    assert np.array_equal(m["xyz"], v) and np.array_equal(m["normals"], R.frustum_normals())
    assert np.array_equal(m["faces"], R.FRUSTUM_TRIANGLES) and (m["rgb"] == 7).all()
    head = open(tmp_path / "m.ply", "rb").read(400).split(b"end_header")[0].decode()
    assert "format binary_little_endian 1.0" in head and "property list uchar int vertex_indices" in head


@pytest.mark.parametrize("tag", ["track", "plain"])
def test_file_list_and_keys_equal_the_reference(gold, tag):
    _, prov = gold
    want = prov["returns"][tag]
    T = prov["T"]
    got = R.ply_list("scene", os.path.join("OUT", "scene"), T, tag == "track")
    assert got == want
    assert np.array_equal(np.array(prov["intrinsics_b44t_after"], np.float32),
                          RS.scene_tensors(_scene({k: v for k, v in np.load(GOLD + ".npz").items()}))[1]
                          ["traj3d_intrinsics_est_b16t"].reshape(1, 4, 4, T).numpy())


def test_restated_nearest_index_equals_grid_sample_on_the_cpu_for_plain_coordinates():
    """The restatement's index rule against ATen on coordinates away from the .5 boundaries (the GPU test covers the boundaries
    against ATen's device kernel, which is what the reference runs)."""
    g = torch.Generator().manual_seed(3)
    H, W = 7, 9
    img = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W) + 1
    xy = torch.rand(200, 2, generator=g) * torch.tensor([W + 4.0, H + 4.0]) - 2
    ix, iy = RS.nearest_index(xy[:, 0], W), RS.nearest_index(xy[:, 1], H)
    ok = ((ix - (((xy[:, 0] / (W - 1) * 2 - 1) + 1) * W - 1) / 2).abs() < 0.49) & ((iy - (((xy[:, 1] / (H - 1) * 2 - 1) + 1) * H - 1) / 2).abs() < 0.49)
    grid = torch.stack([xy[:, 0] / (W - 1) * 2 - 1, xy[:, 1] / (H - 1) * 2 - 1], -1).reshape(1, 1, -1, 2)
    s = torch.nn.functional.grid_sample(img, grid, mode="nearest", align_corners=False).reshape(-1)
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    want = torch.where(inside, img.reshape(-1)[(iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1)).long()], torch.zeros(()))
    assert torch.equal(s[ok], want[ok])
