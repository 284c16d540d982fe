"""Score the engine against ground truth: a directory of .npz clips -> model.test_step -> the metrics of l4p_amd/metrics.py.

Each .npz holds one clip as a dataset's __getitem__ yields it: arrays under the L4PData field names WITHOUT the batch dimension
(rgb_b3thw [3, T, H, W], depth_b1thw [1, T, H, W], depth_valid_b1thw, flow_2d_backward_b2thw, dyn_mask_b1thw, track_2d_traj_bn2t
[N, 2, T], track_2d_vis_bn1t [N, 1, T], track_2d_valid_bn1t, track_2d_pointquerries_bn3 [N, 3], intrinsics_b44t / extrinsics_b44t
[4, 4, T], ...).  ``npz_to_batch`` adds the batch dimension; a task is scored when its ground truth is there.

Prints one JSON line per clip (the scalars of that clip) and one with the mean of each metric over the clips that have a value.

  python tools/evaluate.py CLIPS_DIR --ckpt model.ckpt [--precision 16-mixed] [--depth-align median|none|lstsq]
  python tools/evaluate.py CLIPS_DIR --synthetic [--mini]      # seeded weights, as demo/demo.py --synthetic: plumbing, not numbers
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("clips", help="directory of .npz clips")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "model.yaml"))
    ap.add_argument("--synthetic", action="store_true", help="seeded weights instead of a checkpoint")
    ap.add_argument("--mini", action="store_true", help="with --synthetic: the mini geometry of the test-suite")
    ap.add_argument("--max-queries", type=int, default=128)
    ap.add_argument("--precision", default="16-mixed")
    ap.add_argument("--depth-align", default="median", choices=["median", "none", "lstsq"])
    args = ap.parse_args()
    if not args.synthetic and not args.ckpt:
        ap.error("--ckpt (or --synthetic)")
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
    model.metrics_module = L4PMetrics(depth_align=args.depth_align)
    rows = []
    for i, f in enumerate(files):
        with np.load(f, allow_pickle=False) as z:
            batch = npz_to_batch(z)
        batch.setdefault("seq_name", [os.path.splitext(os.path.basename(f))[0]])
        with torch.no_grad():
            model.test_step(batch, i)
        row = clip_scalars(model.last_log)
        rows.append(row)
        print(json.dumps({"clip": batch["seq_name"][0], **row}))
    print(json.dumps({"clips": len(rows), "mean": mean_over_clips(rows)}))


if __name__ == "__main__":
    main()
