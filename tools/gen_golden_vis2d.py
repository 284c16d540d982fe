"""Generate tests/golden/vis2d_T24.npz (+ .json provenance) from the REFERENCE's own generate_video_visualizations
(l4p/utils/vis.py:34-104), where the reference tree is importable (--ref).

cv2, mediapy and open3d are not installed where this runs: mediapy and open3d are import stand-ins that do nothing, matplotlib 3.10 no
longer has cm.get_cmap (shimmed to matplotlib.colormaps[...]), and cv2 is a stand-in that RECORDS every line / circle /
addWeighted call (points, colour, weights) and draws nothing - so the reference's track panel comes back as its grey background
and the fixture pins the call sequence, not cv2's pixels.  The scene is tests/vis2d_restate.make_scene (stored as the small
integer arrays it is built from).  The integer-valued panels are stored as integers for every frame (depth: entry of the flipped
turbo table, flow: levels of 255, mask: bits), the f32 RGB panel and the grey background for frames KEEP.

  python tools/gen_golden_vis2d.py --ref DIR
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP = (0, 1, 17, 23)
LINE, BLEND, CIRCLE = 0, 1, 2


def install_stubs(ref: str, calls: list):
    import matplotlib
    import matplotlib.cm

    if not hasattr(matplotlib.cm, "get_cmap"):
        matplotlib.cm.get_cmap = matplotlib.colormaps.__getitem__
    sys.modules["mediapy"] = types.ModuleType("mediapy")
    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(TriangleMesh=object, PointCloud=object)  # (named in the 4D helpers' annotations only)
    sys.modules["open3d"] = o3d
    cv2 = types.ModuleType("cv2")
    cv2.LINE_AA = 16

    def line(img, p1, p2, color, thickness, line_type):
        assert thickness == 1 and line_type == cv2.LINE_AA
        calls.append((LINE, [*p1, *p2], list(color), [0.0, 0.0]))

    def circle(img, c, radius, color, thickness):
        assert radius == 2 and thickness == -1
        calls.append((CIRCLE, [*c, 0, 0], list(color), [0.0, 0.0]))

    def add_weighted(a, alpha, b, beta, gamma):
        assert gamma == 0 and a.shape == b.shape
        calls.append((BLEND, [0, 0, 0, 0], [0.0, 0.0, 0.0], [alpha, beta]))
        return a

    cv2.line, cv2.circle, cv2.addWeighted = line, circle, add_weighted
    sys.modules["cv2"] = cv2
    sys.path.insert(0, ref)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (NVlabs/L4P)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vis2d_T24.npz"))
    args = ap.parse_args()
    calls = []
    install_stubs(args.ref, calls)
    import torch
    from l4p.utils.vis import generate_video_visualizations  # the reference's (args.ref is first on sys.path)

    spec = importlib.util.spec_from_file_location("scene", os.path.join(ROOT, "tests", "vis2d_restate.py"))
    sys.path.insert(0, ROOT)  # the module's engine imports resolve to the repository's l4p_amd
    scene = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scene)
    from l4p_amd.utils.vis2d import turbo_table

    sc = scene.make_scene()
    batch, out = scene.scene_tensors(sc)
    vid, name = generate_video_visualizations(batch, out, scene.TASKS)
    _, T, H, W = sc["rgb_u8"].shape
    assert name is None and vid.dtype == np.float32 and vid.shape == (T, H, 5 * W, 3), (vid.dtype, vid.shape)
    rgb, depth, flow, mask, track = (vid[:, :, p * W:(p + 1) * W] for p in range(5))
    table = turbo_table()[::-1].astype(np.float32)
    index_of = {row.tobytes(): k for k, row in enumerate(table)}
    assert len(index_of) == 256
    depth_index = np.array([index_of[px.tobytes()] for px in depth.reshape(-1, 3)], np.uint8).reshape(T, H, W)
    flow_level = np.rint(flow * 255).astype(np.uint8)
    assert np.array_equal(flow_level.astype(np.float32) / np.float32(255), flow)
    assert np.isin(mask, (0.0, 1.0)).all() and (mask[..., 0] == mask[..., 1]).all() and (mask[..., 0] == mask[..., 2]).all()
    assert (track[..., 0] == track[..., 1]).all() and (track[..., 0] == track[..., 2]).all()  # nothing was drawn: the grey video
    keep = list(KEEP)
    arrays = {k: np.asarray(v) for k, v in sc.items()}
    arrays.update(depth_index=depth_index, flow_level=flow_level, mask_bit=np.packbits(mask[..., 0].astype(bool)),
                  rgb_keep=rgb[keep], grey_keep=track[keep][..., 0],
                  call_kind=np.array([c[0] for c in calls], np.int8), call_points=np.array([c[1] for c in calls], np.int32),
                  call_colour=np.array([c[2] for c in calls], np.float64), call_weights=np.array([c[3] for c in calls], np.float64))
    np.savez_compressed(args.out, **arrays)
    prov = {"generator": "tools/gen_golden_vis2d.py", "reference": "NVlabs/L4P l4p/utils/vis.py generate_video_visualizations",
            "stand_ins": ["mediapy (empty)", "open3d (two type names)", "matplotlib.cm.get_cmap", "cv2 (records line / circle / addWeighted, "
                          "draws nothing)"],
            "scene": "tests/vis2d_restate.py make_scene() defaults", "tasks": scene.TASKS, "T": T, "H": H, "W": W,
            "N": int(sc["traj_q"].shape[0]), "keep_frames": keep, "calls": len(calls), "call_kinds": {"line": LINE, "blend": BLEND,
                                                                                                     "circle": CIRCLE},
            "torch": torch.__version__, "numpy": np.__version__}
    with open(os.path.splitext(args.out)[0] + ".json", "w") as f:
        json.dump(prov, f, indent=1)
    print(args.out, os.path.getsize(args.out), "bytes;", len(calls), "calls")


if __name__ == "__main__":
    main()
