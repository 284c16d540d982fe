"""Generate tests/golden/recon4d_T24.npz (+ .json provenance) from the REFERENCE's own generate_4D_visualization
(l4p/utils/vis.py:107-221), where the reference tree is importable (--ref, default /root/reference).

cv2, mediapy and open3d are not installed where this runs: they are replaced by import stand-ins.  The open3d one keeps what
the reference hands it (a PointCloud keeps points / colors and supports +, a TriangleMesh keeps vertices, triangles, colour and
the vertex normals computed as Open3D does; io.write_* records instead of writing).  matplotlib 3.10 no longer has
cm.get_cmap: it is shimmed to matplotlib.colormaps[...].  The scene is tests/recon4d_restate.make_scene (stored as the small
integer arrays it is built from).  Full point arrays are kept for frames KEEP, counts and the scale for every frame.

  python tools/gen_golden_recon4d.py [--ref DIR]
"""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP = (0, 1, 16, 17, 23)


def install_stubs(ref: str, written: dict):
    import matplotlib
    import matplotlib.cm

    if not hasattr(matplotlib.cm, "get_cmap"):
        matplotlib.cm.get_cmap = matplotlib.colormaps.__getitem__
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.modules["mediapy"] = types.ModuleType("mediapy")

    class PointCloud:
        def __init__(self):
            self.points, self.colors = np.zeros((0, 3)), np.zeros((0, 3))

        def __add__(self, o):
            if len(o.points) == 0:
                return self
            r = PointCloud()
            r.points = np.concatenate([np.asarray(self.points, np.float64), np.asarray(o.points, np.float64)])
            r.colors = np.concatenate([np.asarray(self.colors, np.float64), np.asarray(o.colors, np.float64)])
            return r

    class TriangleMesh:
        def __init__(self):
            self.vertices, self.triangles, self.colors, self.normals = None, None, None, None

        def paint_uniform_color(self, c):
            self.colors = np.asarray(c, np.float64)

        def compute_vertex_normals(self):  # Open3D: area-weighted triangle normals summed per vertex, normalised
            v, tri = np.asarray(self.vertices, np.float64), np.asarray(self.triangles)
            fn = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
            n = np.zeros_like(v)
            for k in range(3):
                np.add.at(n, tri[:, k], fn)
            self.normals = n / np.linalg.norm(n, axis=1, keepdims=True)

    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(PointCloud=PointCloud, TriangleMesh=TriangleMesh)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a, np.float64), Vector3iVector=lambda a: np.asarray(a))
    o3d.io = types.SimpleNamespace(write_point_cloud=lambda p, c: written.__setitem__(p, c),
                                   write_triangle_mesh=lambda p, m: written.__setitem__(p, m))
    sys.modules["open3d"] = o3d
    sys.path.insert(0, ref)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "recon4d_T24.npz"))
    args = ap.parse_args()
    written = {}
    install_stubs(args.ref, written)
    import torch
    from l4p.utils.vis import generate_4D_visualization  # the reference's (args.ref is first on sys.path)

    import importlib.util

    spec = importlib.util.spec_from_file_location("scene", os.path.join(ROOT, "tests", "recon4d_restate.py"))
    # make_scene / scene_tensors only: the module's engine imports resolve to the repository's l4p_amd
    sys.path.insert(0, ROOT)
    scene = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scene)
    sc = scene.make_scene()
    T, H, W = sc["depth_q"].shape
    fx = {}
    result = {}
    for tasks in (["depth", "camray", "track_2d"], ["depth", "camray"]):
        batch, out = scene.scene_tensors(sc)
        written.clear()
        ret = generate_4D_visualization(batch, out, tasks, "OUT")
        tag = "track" if "track_2d" in tasks else "plain"
        result[tag] = {"ret": ret, "intrinsics_b44t": batch["intrinsics_b44t"].numpy().tolist()}
        for t in range(T):
            e = ret[t]
            m = written[e["mesh_cam"]]
            pc = written[e["pc_depth_track" if tag == "track" else "pc_depth"]]
            fx.setdefault(f"{tag}_count", []).append(len(pc.points))
            if t in KEEP:
                fx[f"{tag}_xyz_{t}"] = np.asarray(pc.points, np.float32)
                fx[f"{tag}_rgb_{t}"] = np.minimum(255.0, np.maximum(0.0, np.asarray(pc.colors) * 255.0)).astype(np.uint8)
            fx.setdefault(f"{tag}_frustum", []).append(np.asarray(m.vertices, np.float64))
            if t == 0:
                fx[f"{tag}_frustum_normals"] = m.normals
                fx[f"{tag}_frustum_triangles"] = np.asarray(m.triangles, np.int32)
                fx[f"{tag}_frustum_colour"] = m.colors
    # the scale the reference applies (vis.py:160-167), recomputed with its own expression on the same tensors
    batch, out = scene.scene_tensors(sc)
    traj_norm = out["track_2d_traj_est_bn2t"][0].clone()
    traj_norm[:, 0, :] = traj_norm[:, 0, :] / (W - 1) * 2 - 1
    traj_norm[:, 1, :] = traj_norm[:, 1, :] / (H - 1) * 2 - 1
    samp = torch.nn.functional.grid_sample(out["depth_est_b1thw"][0].permute(1, 0, 2, 3), traj_norm.permute(2, 0, 1).unsqueeze(2),
                                           mode="nearest", align_corners=False)[:, 0, :, 0].permute(1, 0)
    vis = torch.sigmoid(out["track_2d_vis_est_bn1t"])[0, :, 0] > 0.75
    scale = torch.median(samp[vis] / out["track_2d_depth_est_bn1t"][0, :, 0][vis])
    arrays = {k: np.asarray(v) for k, v in sc.items()}
    arrays.update({k: np.asarray(v) for k, v in fx.items()})
    arrays["scale"] = np.asarray([scale.item()], np.float32)
    arrays["vis_count"] = vis.sum(0).numpy().astype(np.int32)
    np.savez_compressed(args.out, **arrays)
    prov = {"generator": "tools/gen_golden_recon4d.py", "reference": "NVlabs/L4P l4p/utils/vis.py generate_4D_visualization",
            "stand_ins": ["cv2", "mediapy", "open3d (records, computes vertex normals as Open3D)", "matplotlib.cm.get_cmap"],
            "scene": "tests/recon4d_restate.py make_scene() defaults", "T": T, "H": H, "W": W, "N": int(sc["traj"].shape[0]),
            "keep_frames": list(KEEP), "torch": torch.__version__, "numpy": np.__version__,
            "returns": {k: v["ret"] for k, v in result.items()},
            "intrinsics_b44t_after": result["track"]["intrinsics_b44t"]}
    with open(os.path.splitext(args.out)[0] + ".json", "w") as f:
        json.dump(prov, f, indent=1)
    print(args.out, os.path.getsize(args.out), "bytes; scale", scale.item(), "counts", fx["track_count"])


if __name__ == "__main__":
    main()
