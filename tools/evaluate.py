"""Score the engine against ground truth: a directory of .npz clips -> model.test_step -> the metrics of l4p_amd/metrics.py.

Each .npz holds one clip as a dataset's __getitem__ yields it: arrays under the L4PData field names WITHOUT the batch dimension
(rgb_b3thw [3, T, H, W], depth_b1thw [1, T, H, W], depth_valid_b1thw, flow_2d_backward_b2thw, dyn_mask_b1thw, track_2d_traj_bn2t
[N, 2, T], track_2d_vis_bn1t [N, 1, T], track_2d_valid_bn1t, track_2d_pointquerries_bn3 [N, 3], intrinsics_b44t / extrinsics_b44t
[4, 4, T], ...).  ``npz_to_batch`` adds the batch dimension; a task is scored when its ground truth is there.

Prints one JSON line per clip (the scalars of that clip) and one with the mean of each metric over the clips that have a value.

  python tools/evaluate.py CLIPS_DIR --ckpt model.ckpt [--precision 16-mixed] [--depth-align median|none|lstsq|lstsq_inv]
                           [--depth-log-errors] [--track-3d none|median|track_median|query] [--bidirectional]

--depth-align lstsq_inv fits scale and shift in inverse depth; --depth-log-errors adds depth_sq_rel / rmse_log / log10 / silog;
--track-3d MODE scores the (x, y, z) tracks in camera space (clips with track_2d_depth_bn1t and intrinsics_b44t) with the scale MODE.
--bidirectional tracks every query in both time directions (estimation_directions [1, -1] on the tracker head and, with --raw, on the
dataset, which then leaves track_2d_valid_bn1t as it is): the frames before a query are estimated and scored too.
  python tools/evaluate.py CLIPS_DIR --synthetic [--mini]      # seeded weights, as demo/demo.py --synthetic: plumbing, not numbers

With --raw the .npz files hold RAW clips instead (the dataset's own resolution and length, rgb as float in [0, 1] or uint8): they
go through l4p_amd.data.NpzClipDataset - resize, crop, mirror padding and query filtering on the GPU - and a
DataLoader(batch_size=1) into test_step.  With --raw --synthetic and an empty or missing CLIPS_DIR, two seeded raw clips
(l4p_amd.data.synthetic.synthetic_ground_truth) are written there first.

  python tools/evaluate.py RAW_DIR --raw --resize 224 224 [--crop 16 224 224] [--spacing 0.02] [--seed 0] --ckpt model.ckpt
"""
import argparse
import glob
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STRING_KEYS = ("seq_name", "dataset_name")  # kept as lists of str, as the default collate of a DataLoader leaves them


def npz_to_batch(arrays) -> dict:
    """One unbatched clip (a mapping name -> array, e.g. an open np.load) -> a batch of one clip: every array gains a leading
    dimension of 1 and becomes a tensor (floats as float32, bools and integers as they are), strings become one-element lists."""
    batch = {}
    for key in arrays.keys():
        a = np.asarray(arrays[key])
        if key in STRING_KEYS or a.dtype.kind in "US":
            batch[key] = [str(a.reshape(-1)[0]) if a.size else ""]
            continue
        t = torch.from_numpy(np.ascontiguousarray(a))
        if t.is_floating_point():
            t = t.to(torch.float32)
        batch[key] = t[None]
    return batch


def clip_scalars(log: dict) -> dict:
    """The metric scalars of a step's last_log on the host: {"depth_abs_rel": 0.1, ...} (one device-to-host copy per clip)."""
    keys = [k for k, v in log.items() if torch.is_tensor(v)]
    if not keys:
        return {}
    host = torch.stack([log[k].reshape(()).to(torch.float32) for k in keys]).cpu().tolist()
    return {k.split("/", 2)[2]: v for k, v in zip(keys, host)}


def mean_over_clips(rows) -> dict:
    """Mean of every metric over the clips that have a value for it (NaN where none has)."""
    names = sorted({k for r in rows for k in r})
    out = {}
    for k in names:
        vals = [r[k] for r in rows if k in r and not math.isnan(r[k])]
        out[k] = sum(vals) / len(vals) if vals else float("nan")
    return out


def raw_loader(clips: str, resize, crop, spacing: float, seed: int, directions=(1,)):
    """DataLoader(batch_size=1) over NpzClipDataset(clips): centre crop from the first frame; clips with their own queries keep
    them (scaled with the resize), the others get the uniform grid of ``spacing``."""
    from l4p_amd.data import NpzClipDataset

    torch.manual_seed(seed)
    ds = NpzClipDataset(clips, crop_size=tuple(crop) if crop else None, resize_size=tuple(resize) if resize else None, center_crop=True,
                        start_crop_time=True, estimation_directions=list(directions), track_2d_querry_sampling_version="uniform",
                        track_2d_querry_sampling_spacing=spacing, scale_queries_on_resize=True)
    return torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)


def write_synthetic_raw(clips: str, n: int = 2, T: int = 9, H: int = 56, W: int = 64, N: int = 8):
    os.makedirs(clips, exist_ok=True)
    from l4p_amd.data.synthetic import synthetic_ground_truth

    for i in range(n):
        np.savez(os.path.join(clips, f"synthetic_{i}.npz"), **synthetic_ground_truth(40 + i, T, H, W, N))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("clips", help="directory of .npz clips")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "model.yaml"))
    ap.add_argument("--synthetic", action="store_true", help="seeded weights instead of a checkpoint")
    ap.add_argument("--mini", action="store_true", help="with --synthetic: the mini geometry of the test-suite")
    ap.add_argument("--max-queries", type=int, default=128)
    ap.add_argument("--precision", default="16-mixed")
    ap.add_argument("--depth-align", default="median", choices=["median", "none", "lstsq", "lstsq_inv"])
    ap.add_argument("--depth-log-errors", action="store_true", help="also depth_sq_rel, depth_rmse_log, depth_log10, depth_silog")
    ap.add_argument("--track-3d", default=None, choices=["none", "median", "track_median", "query"], metavar="MODE",
                    help="score the 3D tracks with this scale: none, median (per clip), track_median, query (per track)")
    ap.add_argument("--bidirectional", action="store_true",
                    help="estimation_directions [1, -1]: track, and score, the frames before a query as well")
    ap.add_argument("--raw", action="store_true", help="the .npz files are raw clips: prepare them with NpzClipDataset on the GPU")
    ap.add_argument("--resize", type=int, nargs=2, default=None, metavar=("H", "W"), help="with --raw: resize_size")
    ap.add_argument("--crop", type=int, nargs=3, default=None, metavar=("T", "H", "W"), help="with --raw: crop_size (default: the "
                    "clip's length rounded up to a multiple of 8, at least 16, x 224 x 224)")
    ap.add_argument("--spacing", type=float, default=0.02, help="with --raw: grid spacing of the queries of clips without tracks")
    ap.add_argument("--seed", type=int, default=0, help="with --raw: torch.manual_seed before the clips are drawn")
    args = ap.parse_args(argv)
    if not args.synthetic and not args.ckpt:
        ap.error("--ckpt (or --synthetic)")
    return ap, args


def main():
    ap, args = parse_args()
    if args.raw and args.synthetic and not glob.glob(os.path.join(args.clips, "*.npz")):
        write_synthetic_raw(args.clips)
    files = sorted(glob.glob(os.path.join(args.clips, "*.npz")))
    if not files:
        ap.error(f"no .npz clips under {args.clips}")

    from l4p_amd.metrics import L4PMetrics
    from l4p_amd.models.utils import build_model, prepare_model

    if args.synthetic:
        from l4p_amd.weights import ModelCfg, seeded_state_dict

        cfg = ModelCfg.mini() if args.mini else ModelCfg.full()
        model = build_model(args.config, max_queries=args.max_queries, precision=args.precision, model_cfg=cfg if args.mini else None)
        if args.mini:
            for h in model.l4p_model.task_heads.values():
                if hasattr(h, "hooks_idx"):
                    h.hooks_idx = list(cfg.hooks)
        model.load_state_dict({"l4p_model." + k: v for k, v in seeded_state_dict(cfg).items()})
        model = model.eval()
    else:
        model = prepare_model(model_config_path=args.config, ckpt_path=args.ckpt, max_queries=args.max_queries,
                              precision=args.precision, accelerator="gpu")
    directions = [1, -1] if args.bidirectional else [1]
    if args.bidirectional:
        model.l4p_model.task_heads["track_2d"].estimation_directions = directions
    model.metrics_module = L4PMetrics(depth_align=args.depth_align, track_3d=args.track_3d, depth_log_errors=args.depth_log_errors)
    rows = []

    def batches():
        if args.raw:
            yield from raw_loader(args.clips, args.resize, args.crop, args.spacing, args.seed, directions)
            return
        for f in files:
            with np.load(f, allow_pickle=False) as z:
                batch = npz_to_batch(z)
            batch.setdefault("seq_name", [os.path.splitext(os.path.basename(f))[0]])
            yield batch

    for i, batch in enumerate(batches()):
        with torch.no_grad():
            model.test_step(batch, i)
        row = clip_scalars(model.last_log)
        rows.append(row)
        print(json.dumps({"clip": batch["seq_name"][0], **row}))
    print(json.dumps({"clips": len(rows), "mean": mean_over_clips(rows)}))


if __name__ == "__main__":
    main()
