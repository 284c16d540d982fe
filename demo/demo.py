"""The reference's demo (demo/demo.py:45-258) on the MI355X engine: VideoDataset (--videos, its sections 2 / 4), DavisDataset (--davis,
sections 1 / 3) or DycheckDataset (--dycheck, section 5: the camera file's intrinsics, use_intrinsics=True) ->
DataLoader(batch_size=1) -> prepare_model(...).forward(batch, tasks).  The outputs are reported (and optionally saved as .npz).
--vis DIR writes the reference's side-by-side result video (generate_video_visualizations, demo.py:78,113: RGB, depth, flow, motion
mask, track trails) rendered on the GPU; --recon4d DIR adds the camray task and writes the 4D reconstruction of the reference's 4D
sections (generate_4D_visualization, demo.py:116-258) as PLY files under DIR; --view4d DIR adds the camray task too and renders what
those sections end in (visualize_point_cloud_viser, demo.py:151-160: the point cloud of frame t, track trails and camera frustum from a
free viewpoint) on the GPU, along an orbit camera path, as a video under DIR.  --scene-flow DIR (this project's own, no counterpart
in the reference) adds the camray task as well and combines depth, flow and pose across time: per-pixel 3D motion in the world frame
and the flow split into its camera-induced and its object part (l4p_amd.utils.scene_flow), as .npz, consistency numbers as .json and
an [RGB | flow | camera-compensated flow] video; with --view4d the 4D video is rendered once more, coloured by 3D speed.
--static-map DIR (this project's own as well) adds the camray task and fuses the clip's per-frame point clouds into ONE voxel map of
the static scene (l4p_amd.utils.static_map): a PLY of the voxels seen in at least two frames and outside the motion mask, and its
counters as .json.
--objects DIR (this project's own too) adds the camray task and labels the motion mask into moving objects over space-time
(l4p_amd.utils.moving_objects): per-object boxes, centroids and speeds as .json, the objects' world points as .ply and an overlay video.
--object-models DIR (this project's own too) adds the camray task and fits every moving object's rigid motion per frame, then fuses
the object's points of all frames into ONE model in the pose of its first frame (l4p_amd.utils.object_motion): the models as .ply,
the motions, poses and fit counters as .json.
--native DIR (this project's own, --videos / --synthetic) carries the dense results from the network's 224 x 224 grid to the pixel
grid of the decoded video by guided up-sampling on the GPU (l4p_amd.utils.native_res): depth, flow in source pixels, mask logits,
validity and the mapped tracks as <seq_name>_native.npz; with --vis also the five-panel video at the source resolution.

  python demo/demo.py --videos a.mp4 b.mp4 --ckpt weights/l4p_depth_flow_2d3dtrack_camray_dynseg_v1.ckpt   # needs mediapy
  python demo/demo.py --synthetic                      # no checkpoint / video files here: seeded weights + a seeded video
  python demo/demo.py --synthetic --vis out/           # + the five-panel result video (.mp4 with mediapy, PNG frames without)
  python demo/demo.py --synthetic --recon4d out/       # + 4D point clouds / track trails / frusta as PLY under out/
  python demo/demo.py --synthetic --view4d out/        # + the 4D result from a free viewpoint (.mp4 with mediapy, PNG frames without)
  python demo/demo.py --synthetic --scene-flow out/    # + scene flow / camera-compensated flow (.npz, .json, video) under out/
  python demo/demo.py --synthetic --static-map out/    # + one fused voxel map of the static scene (.ply, .json) under out/
  python demo/demo.py --synthetic --objects out/       # + the moving objects of the clip (.json, .ply, overlay video) under out/
  python demo/demo.py --synthetic --object-models out/ # + one fused model per moving object and its motion (.ply, .json) under out/
  python demo/demo.py --synthetic --native out/ --vis out/   # + depth / flow / mask at the video's own resolution (.npz, video) under out/
  python demo/demo.py --davis DAVIS_ROOT --ckpt ...    # JPEGImages/480p/<seq>, Annotations/480p/<seq>: queries on the instance masks
  python demo/demo.py --dycheck DYCHECK_ROOT --ckpt ... --recon4d out/   # <seq>/dense/images, <seq>/calibration.txt
  python demo/demo.py --synthetic --davis X --vis out/ # a small seeded DAVIS (or --dycheck: DyCheck) tree in a temporary directory
  python demo/demo.py --synthetic --frames 32 --bidirectional --query-frame 12 --vis out/   # queries on frame 12, tracked both ways

With --synthetic the weights are the name-seeded random tensors of the test-suite (same 916-key state dict a checkpoint
holds) and the "video" is l4p_amd.data.synthetic.synthetic_video: the point is the plumbing and the timing, not the pictures.
"""
import argparse
import contextlib
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from l4p_amd.data import DavisDataset, DycheckDataset, VideoDataset
from l4p_amd.models.utils import build_model, prepare_model


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", nargs="*", default=[])
    ap.add_argument("--davis", default=None, metavar="ROOT",
                    help="a DAVIS tree (the reference demo's sections 1 / 3): queries sampled on the instance masks at spacing 0.02; "
                         "with --recon4d the crop is (56, 224, 224).  With --synthetic: a seeded tree in a temporary directory")
    ap.add_argument("--dycheck", default=None, metavar="ROOT",
                    help="a DyCheck tree (section 5): resize (298, 224), stride 2, spacing 0.04, camray with the camera file's "
                         "intrinsics (use_intrinsics=True).  With --synthetic: a seeded tree in a temporary directory")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "model.yaml"))
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--frames", type=int, default=64, help="crop_size[0] (the demo uses 64, or 16 to limit memory)")
    ap.add_argument("--max-queries", type=int, default=128)
    ap.add_argument("--spacing", type=float, default=None,
                    help="track_2d_querry_sampling_spacing (default 0.04 = 625 queries; 0.02 for --davis, as the reference demo)")
    ap.add_argument("--save", default=None, help="directory for <seq_name>.npz")
    ap.add_argument("--vis", default=None, metavar="DIR",
                    help="write each video's 2D result video (RGB | depth | flow | motion mask | tracks; "
                         "l4p_amd.utils.vis2d.generate_video_visualizations) under DIR")
    ap.add_argument("--recon4d", default=None, metavar="DIR",
                    help="also run the camray task and write each video's 4D reconstruction (world point clouds, 3D track trails, "
                         "camera frusta as PLY; l4p_amd.utils.recon4d.generate_4D_visualization) under DIR")
    ap.add_argument("--view4d", default=None, metavar="DIR",
                    help="also run the camray task and render each video's 4D reconstruction from an orbiting viewpoint (points, track "
                         "trails, camera frusta; l4p_amd.utils.view4d.generate_4D_video) as <seq_name>_4d under DIR")
    ap.add_argument("--scene-flow", default=None, metavar="DIR", dest="scene_flow",
                    help="also run the camray task and write each video's dense scene flow, rigid and camera-compensated flow "
                         "(<seq_name>_sceneflow.npz), their consistency numbers (.json) and an RGB | flow | compensated-flow video "
                         "(l4p_amd.utils.scene_flow) under DIR; with --view4d also <seq_name>_4d_motion, the 4D video coloured by 3D speed")
    ap.add_argument("--static-map", default=None, metavar="DIR", dest="static_map",
                    help="also run the camray task and fuse each video's per-frame point clouds into one voxel map of the static scene "
                         "(<seq_name>_static_map.ply, its counters as .json; l4p_amd.utils.static_map.generate_static_map) under DIR")
    ap.add_argument("--objects", default=None, metavar="DIR",
                    help="also run the camray task and label the motion mask into moving objects over space-time, frames linked through "
                         "the backward flow (<seq_name>_objects.json: counters and per-object boxes, centroids and speeds; .ply: the objects' "
                         "world points; an overlay video; l4p_amd.utils.moving_objects.generate_moving_objects) under DIR")
    ap.add_argument("--object-models", default=None, metavar="DIR", dest="object_models",
                    help="also run the camray task, fit every moving object's rigid motion per frame from its flow-linked pixel pairs and "
                         "fuse its points of all frames into one model (<seq_name>_object_models.ply, <seq_name>_object_motion.json; "
                         "l4p_amd.utils.object_motion.generate_object_models) under DIR")
    ap.add_argument("--native", default=None, metavar="DIR",
                    help="(--videos / --synthetic) write each video's depth, flow (in source pixels), mask logits, validity and tracks at "
                         "the resolution of the decoded frames (<seq_name>_native.npz; guided up-sampling, l4p_amd.utils.native_res) under "
                         "DIR; with --vis also the five-panel video at that resolution as <seq_name>_native")
    ap.add_argument("--synthetic-size", type=int, nargs=2, default=(480, 854), metavar=("H", "W"), dest="synthetic_size",
                    help="frame size of the seeded --synthetic video (default 480 854)")
    ap.add_argument("--bidirectional", action="store_true",
                    help="track every query in both time directions (estimation_directions [1, -1] on the tracker head and the dataset): "
                         "the frames before a query are estimated by a second tracker pass over the time-flipped clip")
    ap.add_argument("--query-frame", type=int, default=None, metavar="K",
                    help="place the sampled queries on frame K (time K + 0.5) instead of frame 0, where the datasets sample them")
    ap.add_argument("--precision", default="16-mixed",
                    help="engine: 16-mixed (the reference demo's own, IEEE half; default) | bf16 (what bench.py measures) | 32-true")
    args = ap.parse_args(argv)
    if sum(bool(v) for v in (args.videos, args.davis, args.dycheck)) > 1:
        ap.error("--videos, --davis and --dycheck are one input each: give one")
    if not args.synthetic and not (args.ckpt and (args.videos or args.davis or args.dycheck)):
        ap.error("--ckpt and one of --videos / --davis / --dycheck (or --synthetic)")
    if args.native and (args.davis or args.dycheck):
        ap.error("--native: the --videos / --synthetic flow (VideoDataset.source_clip)")
    if args.query_frame is not None and args.query_frame < 0:
        ap.error("--query-frame: a frame index >= 0")
    if args.spacing is None:
        args.spacing = 0.02 if args.davis else 0.04  # demo.py:50,133 / :88,221
    return args


def plan(args):
    """(tasks, dataset keyword arguments) of the reference demo's section that ``args`` selects."""
    tasks = ["depth", "flow_2d_backward", "dyn_mask", "track_2d"]  # demo.py:82,99
    if args.recon4d or args.view4d or args.dycheck or args.scene_flow or args.static_map or args.objects or args.object_models:
        tasks.append("camray")  # the reference's 4D sections (demo.py:116-258) add it; scene flow, the static map and the objects' 3D tables
        # need the poses too
    kw = dict(crop_size=(args.frames, 224, 224), estimation_directions=[1, -1] if args.bidirectional else [1],
              track_2d_querry_sampling_spacing=args.spacing)
    if args.davis and (args.recon4d or args.view4d):
        kw["crop_size"] = (56, 224, 224)  # demo.py:131
    if args.dycheck:
        kw.update(resize_size=(298, 224), stride=2)  # demo.py:216-224
    return tasks, kw


def synthetic_tree(args, tmp):
    """--synthetic --davis / --dycheck: a small seeded tree (PNG-encoded frames, palette masks, a calibration.txt) under ``tmp``."""
    from l4p_amd.data.synthetic import synthetic_masks, synthetic_video, write_davis_tree, write_dycheck_tree

    if args.davis:
        frames = synthetic_video(1, 20, 120, 214)
        return write_davis_tree(os.path.join(tmp, "davis"), "synthetic", frames, synthetic_masks(2, 20, 120, 214, "blob"), "P")
    frames = synthetic_video(1, 24, 181, 135)
    return write_dycheck_tree(os.path.join(tmp, "dycheck"), "synthetic", frames, (403.217, 398.06, 66.9, 91.325))


def main(argv=None):
    args = parse_args(argv)
    precision, accelerator = args.precision, "gpu"  # demo.py:22-23 hard-codes "16-mixed"
    tasks, kw = plan(args)
    frames = None
    if args.synthetic:
        from l4p_amd.weights import ModelCfg, seeded_state_dict
        from l4p_amd.data.synthetic import synthetic_video

        model = build_model(args.config, max_queries=args.max_queries, precision=precision)
        model.load_state_dict({"l4p_model." + k: v for k, v in seeded_state_dict(ModelCfg.full()).items()})
        model = model.eval()
        if not (args.davis or args.dycheck):
            args.videos = ["synthetic/480p.mp4"]
            frames = {args.videos[0]: synthetic_video(1, 50, *args.synthetic_size)}
    else:
        model = prepare_model(model_config_path=args.config, ckpt_path=args.ckpt, max_queries=args.max_queries,
                              precision=precision, accelerator=accelerator)

    model.l4p_model.window_batch = 8  # windows of a long clip go through encoder + dense decoders eight at a time
    if args.bidirectional:
        model.l4p_model.task_heads["track_2d"].estimation_directions = [1, -1]
    with contextlib.ExitStack() as stack:
        if args.synthetic and (args.davis or args.dycheck):
            root = synthetic_tree(args, stack.enter_context(tempfile.TemporaryDirectory()))
        else:
            root = args.davis or args.dycheck
        if args.davis:
            dataset = DavisDataset(data_root=root, **kw)
        elif args.dycheck:
            dataset = DycheckDataset(data_root=root, **kw)
        else:
            dataset = VideoDataset(video_paths=args.videos, frames=frames, **kw)
        camray = model.l4p_model.task_heads["camray"] if "camray" in tasks else None
        saved = camray.use_intrinsics if camray is not None else None
        if args.dycheck:
            camray.use_intrinsics = True  # demo.py:226: pose from the rays and the INPUT intrinsics
        try:
            run(args, model, dataset, tasks)
        finally:
            if args.dycheck:
                camray.use_intrinsics = saved  # demo.py:258


def run(args, model, dataset, tasks):
    loader = torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False)
    for index, batch in enumerate(loader):
        if args.query_frame is not None:
            if args.query_frame >= batch["rgb_b3thw"].shape[2]:
                raise SystemExit(f"--query-frame {args.query_frame}: the clip has {batch['rgb_b3thw'].shape[2]} frames")
            batch["track_2d_pointquerries_bn3"][..., 0] = args.query_frame + 0.5
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = model.forward(batch, tasks)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        T = batch["rgb_b3thw"].shape[2]
        print(f"{batch['seq_name'][0]}: {T} frames, {batch['track_2d_pointquerries_bn3'].shape[1]} queries, "
              f"{dt * 1e3:.1f} ms ({T / dt:.1f} frames/s)")
        for k, v in out.items():
            if torch.is_tensor(v):
                print(f"  {k:32s} {tuple(v.shape)} {v.dtype}")
        if args.save:
            os.makedirs(args.save, exist_ok=True)
            np.savez_compressed(os.path.join(args.save, os.path.splitext(batch["seq_name"][0])[0] + ".npz"),
                                **{k: v.float().cpu().numpy() for k, v in out.items() if torch.is_tensor(v)})
        if args.vis:
            vis_2d(batch, out, tasks, args.vis)
        if args.recon4d:
            recon_4d(batch, out, tasks, args.recon4d)
        if args.view4d:
            view_4d(batch, out, tasks, args.view4d)
        if args.scene_flow:
            scene_flow(batch, out, tasks, args.scene_flow, view4d_dir=args.view4d)
        if args.static_map:
            static_map(batch, out, tasks, args.static_map)
        if args.objects:
            objects(batch, out, tasks, args.objects)
        if args.object_models:
            object_models(batch, out, tasks, args.object_models)
        if args.native:
            native(batch, out, tasks, *dataset.source_clip(index), args.native, vis_dir=args.vis)


def vis_2d(batch, out, tasks, out_dir):
    """generate_video_visualizations split into its GPU part (render + the one copy to the host) and its file writing, each timed on
    its own."""
    from l4p_amd.utils import vis2d

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = vis2d.render_video_panels(batch, out, tasks)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    vid = res["video"].cpu().numpy()
    t2 = time.perf_counter()
    name = vis2d.write_video(vid, out_dir, batch["seq_name"][0])
    t3 = time.perf_counter()
    lo, hi = res["depth_range"].tolist()
    panels = vid.shape[2] // batch["rgb_b3thw"].shape[-1]
    print(f"  2D: {vid.shape[0]} frames of {panels} panels, depth range {lo:.3g} .. {hi:.3g}, flow radius "
          f"{float(res['flow_rad_max'][0]):.3g}; GPU render {(t1 - t0) * 1e3:.1f} ms, copy to host {(t2 - t1) * 1e3:.1f} ms, file writing "
          f"{(t3 - t2) * 1e3:.0f} ms -> {name}")


def recon_4d(batch, out, tasks, out_dir):
    """generate_4D_visualization split into its GPU part and its file writing, each timed on its own.  (With --synthetic the
    seeded weights give an arbitrary, possibly ill-conditioned K: the files are written, the geometry means nothing.)"""
    from l4p_amd.utils import recon4d

    T, H, W = batch["rgb_b3thw"].shape[2:]
    seq = batch["seq_name"][0]
    path = os.path.join(out_dir, seq)
    os.makedirs(path, exist_ok=True)
    batch["intrinsics_b44t"] = out["traj3d_intrinsics_est_b16t"].reshape(1, 4, 4, T)  # vis.py:126-127
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = recon4d.reconstruct_4d(batch, out, tasks)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    recon4d.write_4d_files(rec, seq, path, T, H * W, "track_2d" in tasks)
    t2 = time.perf_counter()
    n = rec["points"].shape[0] + rec.get("track_xyz", rec["points"][:0]).shape[0]
    print(f"  4D: {T} frames, {n / 1e6:.2f} M points, scale {float(rec.get('scale', torch.ones(1))[0]):.4g}; "
          f"GPU reconstruction {(t1 - t0) * 1e3:.1f} ms, PLY writing {(t2 - t1) * 1e3:.0f} ms -> {path}")


def view_4d(batch, out, tasks, out_dir, colors=None, suffix="_4d"):
    """generate_4D_video split into its GPU part (reconstruction, camera path, renderer), the copy to the host and the file writing,
    each timed on its own.  ``colors`` (uint8 [T H W, 3] on the device) replaces the reconstruction's point colours."""
    from l4p_amd.utils import recon4d, view4d, vis2d

    T, H, W = batch["rgb_b3thw"].shape[2:]
    size = (480, 640)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = recon4d.reconstruct_4d(batch, out, tasks)
    if colors is not None:
        rec["colors"] = colors
    path = view4d.orbit_views(rec, out["depth_est_b1thw"], T, T)
    K = out["traj3d_intrinsics_est_b16t"].reshape(4, 4, T)[:, :, 0].float().cpu().numpy().astype(np.float64)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    res = view4d.render_4d_views(rec, T, H * W, path["cam_T_world"], view4d.scaled_intrinsics(K, (H, W), size), size, path["frames"],
                                 tracks="track_2d" in tasks)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    frames = res["image"].cpu().numpy()
    t3 = time.perf_counter()
    name = vis2d.write_video(frames, out_dir, batch["seq_name"][0] + suffix)
    t4 = time.perf_counter()
    print(f"  4D view: {frames.shape[0]} views of {size[0]} x {size[1]}, look-at distance {path['d0']:.3g}; reconstruction + camera path "
          f"{(t1 - t0) * 1e3:.1f} ms, GPU render {(t2 - t1) * 1e3:.1f} ms, copy to host {(t3 - t2) * 1e3:.1f} ms, file writing "
          f"{(t4 - t3) * 1e3:.0f} ms -> {name}")


def scene_flow(batch, out, tasks, out_dir, view4d_dir=None):
    """Scene flow, rigid and camera-compensated flow of the clip (l4p_amd.utils.scene_flow): <seq>_sceneflow.npz (the four fields, the
    scene flow as float16), <seq>_sceneflow.json (the consistency numbers; NaN where a class has no pixel) and the
    [RGB | flow | camera-compensated flow] video <seq>_sceneflow.  With ``view4d_dir`` the 4D video is rendered a second time as
    <seq>_4d_motion, its points coloured by 3D speed.  (With --synthetic the seeded weights give arbitrary poses and intrinsics: the
    files are written, the numbers mean nothing.)"""
    import json

    from l4p_amd.utils import scene_flow as sf

    seq = batch["seq_name"][0]
    H, W = batch["rgb_b3thw"].shape[-2:]
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = sf.scene_flow_from_outputs(batch, out, tasks)
    numbers = sf.consistency(res["summary_bt8"], pixels_per_frame=H * W)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    np.savez_compressed(os.path.join(out_dir, seq + "_sceneflow.npz"),
                        scene_flow_backward_b3thw=res["scene_flow_backward_b3thw"].cpu().numpy().astype(np.float16),
                        rigid_flow_2d_backward_b2thw=res["rigid_flow_2d_backward_b2thw"].cpu().numpy(),
                        compensated_flow_2d_backward_b2thw=res["compensated_flow_2d_backward_b2thw"].cpu().numpy(),
                        scene_flow_valid_b1thw=res["scene_flow_valid_b1thw"].cpu().numpy())
    numbers = {k: float(v[0]) for k, v in numbers.items()}
    with open(os.path.join(out_dir, seq + "_sceneflow.json"), "w") as fh:
        json.dump(numbers, fh, indent=1)  # NaN is written as NaN (Python's json reads it back)
    _, name = sf.generate_scene_flow_video(batch, out, tasks, out_dir, res=res)
    t2 = time.perf_counter()
    print(f"  scene flow: static rigid EPE {numbers['rigid_epe_static']:.3g} px, dynamic {numbers['rigid_epe_dynamic']:.3g} px, moving "
          f"fraction {numbers['moving_fraction']:.3g}, valid fraction {numbers['valid_fraction']:.3g}; GPU {(t1 - t0) * 1e3:.1f} ms, "
          f"files {(t2 - t1) * 1e3:.0f} ms -> {name}")
    if view4d_dir:
        view_4d(batch, out, tasks, view4d_dir, colors=sf.motion_colors(res)[0], suffix="_4d_motion")


def static_map(batch, out, tasks, out_dir):
    """The clip's point clouds fused into one voxel map of the static scene (l4p_amd.utils.static_map): <seq>_static_map.ply and
    <seq>_static_map.json, the GPU part and the file writing timed on their own.  (With --synthetic the seeded weights give arbitrary
    poses and depths: the files are written, the map means nothing.)"""
    from l4p_amd.utils import static_map as sm

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = sm.static_map_from_outputs(batch, out, tasks)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    name = sm.generate_static_map(batch, out, tasks, out_dir, res=res)
    t2 = time.perf_counter()
    c = res["counters"]
    ratio = c["n_used"] / c["n_kept"] if c["n_kept"] else float("nan")
    print(f"  static map: {c['n_kept']} of {c['n_voxels']} voxels of {float(res['grid'][3]):.3g} kept, {c['n_used']} of {c['n_points']} "
          f"points used ({c['n_masked']} masked), {ratio:.1f} points per voxel; GPU {(t1 - t0) * 1e3:.1f} ms, files "
          f"{(t2 - t1) * 1e3:.0f} ms -> {name}")


def objects(batch, out, tasks, out_dir):
    """The motion mask labelled into moving objects (l4p_amd.utils.moving_objects): <seq>_objects.json, <seq>_objects.ply and the overlay
    video <seq>_objects, the GPU part and the file writing timed on their own.  (With --synthetic the seeded weights give an arbitrary
    mask: the files are written, the objects mean nothing.)"""
    from l4p_amd.utils import moving_objects as mo

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = mo.moving_objects_from_outputs(batch, out, tasks)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    name = mo.generate_moving_objects(batch, out, tasks, out_dir, res=res)
    t2 = time.perf_counter()
    c = res["counters"]
    fastest = float(res["speed"].max()) if "speed" in res and res["K"] else float("nan")
    on = int((res["track_object"] >= 0).sum()) if "track_object" in res else 0
    print(f"  objects: {c['n_kept']} of {c['n_components']} components kept, {c['n_kept_pixels']} of {c['n_foreground']} foreground pixels "
          f"({c['n_pixels']} in all), fastest step {fastest:.3g}, {on} tracks on objects; GPU {(t1 - t0) * 1e3:.1f} ms, files "
          f"{(t2 - t1) * 1e3:.0f} ms -> {name}")


def object_models(batch, out, tasks, out_dir):
    """Every moving object's rigid motion per frame and its fused model (l4p_amd.utils.object_motion): <seq>_object_models.ply and
    <seq>_object_motion.json, the GPU part and the file writing timed on their own.  (With --synthetic the seeded weights give an
    arbitrary mask: the files are written, the models mean nothing.)"""
    from l4p_amd.utils import object_motion as om

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = om.object_motion_from_outputs(batch, out, tasks)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    name = om.generate_object_models(batch, out, tasks, out_dir, res=res)
    t2 = time.perf_counter()
    mo, md = res["motion"], res["models"]
    rows = int(mo["valid"].sum()) if res["K"] else 0
    print(f"  object models: {res['K']} objects, {rows} valid motions of {int((mo['n_pairs'] > 0).sum()) if res['K'] else 0} rows with pairs, "
          f"{md['offsets'][-1]} model vertices from {res['counters']['n_kept_pixels']} object pixels; GPU {(t1 - t0) * 1e3:.1f} ms, files "
          f"{(t2 - t1) * 1e3:.0f} ms -> {name}")


def native(batch, out, tasks, frames, geometry, out_dir, vis_dir=None):
    """The dense results at the resolution of the decoded frames (l4p_amd.utils.native_res): <seq>_native.npz (depth, flow in source
    pixels and mask logits as float16, validity, the mapped tracks), the GPU part and the file writing timed on their own.  With
    ``vis_dir`` the five-panel video is rendered once more at the source resolution as <seq>_native."""
    from l4p_amd.utils import native_res as nr
    from l4p_amd.utils import vis2d

    seq = batch["seq_name"][0]
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = nr.native_resolution_outputs(batch, out, tasks, frames, geometry)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    keys = [k for k in ("depth_est_b1thw", "flow_2d_backward_est_b2thw", "dyn_mask_est_b1thw") if k in res]
    arrays = {k: res[k].cpu().numpy().astype(np.float16) for k in keys}
    arrays["native_valid_b1thw"] = res["native_valid_b1thw"].cpu().numpy()
    if "track_2d_traj_est_bn2t" in res:
        arrays["track_2d_traj_est_bn2t"] = res["track_2d_traj_est_bn2t"].cpu().numpy()
    np.savez_compressed(os.path.join(out_dir, seq + "_native.npz"), **arrays)
    t2 = time.perf_counter()
    H, W = geometry.src_hw
    print(f"  native: {len(keys)} fields at {H} x {W} from {geometry.out_hw[0]} x {geometry.out_hw[1]}, valid fraction "
          f"{float(arrays['native_valid_b1thw'].mean()):.3g}; GPU {(t1 - t0) * 1e3:.1f} ms, files {(t2 - t1) * 1e3:.0f} ms -> "
          f"{os.path.join(out_dir, seq + '_native.npz')}")
    if vis_dir:
        t3 = time.perf_counter()
        vid = vis2d.render_video_panels(nr.native_batch(batch, frames, geometry), res, tasks)["video"]
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        name = vis2d.write_video(vid.cpu().numpy(), vis_dir, seq + "_native")
        t5 = time.perf_counter()
        print(f"  native 2D: {vid.shape[0]} frames of {vid.shape[2] // W} panels at {H} x {W}; GPU render {(t4 - t3) * 1e3:.1f} ms, copy to "
              f"host and file writing {(t5 - t4) * 1e3:.0f} ms -> {name}")


if __name__ == "__main__":
    main()
