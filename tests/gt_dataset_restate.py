"""TEST INFRASTRUCTURE ONLY — CPU restatement (numpy / torch) of the reference's L4PDataset.__getitem__
(l4p/data/l4p_dataset_mini.py:543-587) on raw ground-truth arrays, and the seeded cases of tests/golden/gt_dataset.npz
(tools/gen_golden_gt_dataset.py).

Every stage is materialised, in the reference's order: the mirror padding is iterated on the arrays themselves (:126-190,
:558-560; nothing here knows about frame tables or swap flags), then the resize (:237-290; nearest with ATen's index rule,
trilinear as per-frame bilinear through oracle.preprocess_oracle.interp_axis, un-fused float32), the crop with its draws from
torch's global generator (:292-395), the dummy ground truth (:418-497), the causal valid fix (:499-519) and the normalisation.
float32 throughout, one rounding per operation.
"""
from __future__ import annotations

import hashlib
import math
import os
from typing import Dict, Optional

import numpy as np
import torch

from l4p_amd.data.synthetic import synthetic_ground_truth
from oracle import preprocess_oracle as po
from tests.datasets_restate import torch_nearest_index

F = np.float32
DENSE = ("rgb_b3thw", "depth_b1thw", "depth_valid_b1thw", "instanceseg_b1thw", "dyn_mask_b1thw", "dyn_mask_valid_b1thw",
         "flow_2d_backward_b2thw", "flow_2d_forward_b2thw", "flow_2d_backward_valid_b2thw", "flow_2d_forward_valid_b2thw")
FLOW = ("flow_2d_backward_b2thw", "flow_2d_forward_b2thw", "flow_2d_backward_valid_b2thw", "flow_2d_forward_valid_b2thw")
TRACKS_T = ("track_2d_traj_bn2t", "track_2d_depth_bn1t", "track_2d_vis_bn1t", "track_2d_valid_bn1t")
CAMERAS = ("intrinsics_b44t", "extrinsics_b44t", "rel_pose_b6t")
QUERY = ("track_2d_pointquerries_bn3", "track_2d_pointlabels_bn")
MEAN = np.array([0.485, 0.456, 0.406], dtype=F)
STD = np.array([0.229, 0.224, 0.225], dtype=F)

# name -> raw clip (seed, T0, H, W, N; `drop`: field groups left out of the record), constructor arguments (`ctor`) and the
# torch.manual_seed before ds[0].  Only what differs from the reference's defaults is listed in `ctor`.
_A = dict(raw=dict(seed=3, T=5, H=10, W=14, N=9), drop=(), manual_seed=3)
CASES = {
    # crop only, user queries, both flows; the mirror swap sits inside the crop, the filter drops queries
    "A": dict(_A, ctor=dict(crop_size=(6, 7, 9), estimation_directions=[1])),
    "B": dict(_A, ctor=dict(crop_size=(6, 7, 9), estimation_directions=[-1])),
    "C": dict(_A, ctor=dict(crop_size=(6, 7, 9), estimation_directions=[1, -1])),
    "A_keep": dict(_A, ctor=dict(crop_size=(6, 7, 9), estimation_directions=[1], remove_queries_outside_bounds=False)),
    # resize down + crop, dummy ground truth with random queries
    "D": dict(raw=dict(seed=4, T=5, H=10, W=14, N=9), drop=("tracks",), manual_seed=4,
              ctor=dict(resize_size=(7, 9), crop_size=(6, 5, 6), track_2d_traj_per_sample=5)),
    "D_modes": dict(raw=dict(seed=4, T=5, H=10, W=14, N=9), drop=("tracks",), manual_seed=4,
                    ctor=dict(resize_size=(7, 9), crop_size=(6, 5, 6), track_2d_traj_per_sample=5,
                              resize_mode={"depth_b1thw": "trilinear", "rgb_b3thw": "nearest"})),
    # single frame, up-scaling: the border clamps of both index rules
    "E": dict(raw=dict(seed=5, T=1, H=10, W=14, N=9), drop=("tracks", "flow"), manual_seed=5,
              ctor=dict(resize_size=(23, 19), crop_size=(4, 5, 6), center_crop=True, track_2d_traj_per_sample=3)),
    # crop_size None -> (16, 224, 224): 5 -> 9 -> 17 frames, two mirror rounds
    "F": dict(raw=dict(seed=6, T=5, H=10, W=14, N=9), drop=("tracks",), manual_seed=6,
              ctor=dict(resize_size=(224, 224), crop_size=None, track_2d_traj_per_sample=4, track_2d_querry_sampling_version="uniform",
                        track_2d_querry_sampling_spacing=0.25)),
    # no-op crop: no filter, no visibility clearing although some queries and track points lie outside
    "G": dict(raw=dict(seed=7, T=6, H=7, W=9, N=9), drop=(), manual_seed=7, ctor=dict(crop_size=(6, 7, 9), estimation_directions=[1])),
}
# this engine's extension: no reference exists for it
CASE_J = dict(_A, ctor=dict(crop_size=(6, 7, 9), resize_size=(7, 9), estimation_directions=[1], scale_queries_on_resize=True))


def case_raw(case: dict) -> Dict[str, np.ndarray]:
    """The raw record of a case (numpy arrays under the L4PData names)."""
    raw = synthetic_ground_truth(**case["raw"])
    if "tracks" in case["drop"]:
        for k in TRACKS_T + QUERY:
            raw.pop(k)
    if "flow" in case["drop"]:
        for k in FLOW:
            raw.pop(k)
    return raw


def mirror_once(x: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """mirror_and_pad (:126-190): x -> cat([x, flip(x)[1:]]) along time; a flow field is continued with the OTHER direction."""
    out = {}
    for k, v in x.items():
        if k in FLOW:
            other = k.replace("backward", "forward") if "backward" in k else k.replace("forward", "backward")
            out[k] = np.concatenate([v, x[other][:, ::-1][:, 1:]], axis=1)
        elif k in DENSE:
            out[k] = np.concatenate([v, v[:, ::-1][:, 1:]], axis=1)
        elif k in TRACKS_T + CAMERAS:
            out[k] = np.concatenate([v, v[..., ::-1][..., 1:]], axis=-1)
        else:
            out[k] = v
    return out


def pad(x: Dict[str, np.ndarray], target: int) -> Dict[str, np.ndarray]:
    T0 = x["rgb_b3thw"].shape[1]
    if T0 == 1:  # repeat_single_frame (:192-235)
        out = {}
        for k, v in x.items():
            if k in DENSE:
                out[k] = np.repeat(v, target, axis=1)
            elif k == "extrinsics_b44t":
                out[k] = np.repeat(np.eye(4, dtype=F)[:, :, None], target, axis=2)
            elif k == "rel_pose_b6t":
                out[k] = np.zeros((6, target), dtype=F)
            elif k in TRACKS_T + CAMERAS:
                out[k] = np.repeat(v, target, axis=-1)
            else:
                out[k] = v
        return out
    while x["rgb_b3thw"].shape[1] < target:
        x = mirror_once(x)
    return x


def linear_axis(n_in: int, n_out: int):
    """(i0, i1, w0, w1) of one axis as ATen's linear kernels index it: an axis whose size does not change is "simply copied" with
    i1 = i0 and weights (1, 0) (UpSampleKernel.cpp compute_source_index_and_lambda), every other axis as oracle.preprocess_oracle."""
    if n_in == n_out:
        i = np.arange(n_in, dtype=np.int64)
        return i, i, np.ones(n_in, dtype=F), np.zeros(n_in, dtype=F)
    return po.interp_axis(n_in, n_out)


def bilinear(x: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """F.interpolate(trilinear) with the frame count unchanged: w0 * v0 + w1 * v1 per axis, W inside H inside T, float32, un-fused.
    The time axis is one of the "simply copied" ones: 1 * v + 0 * v, which leaves every finite v as it is and turns inf into nan."""
    H, W = x.shape[-2:]
    y0, y1, wy0, wy1 = linear_axis(H, out_h)
    x0, x1, wx0, wx1 = linear_axis(W, out_w)
    with np.errstate(invalid="ignore"):
        top = (x[:, :, y0][..., x0] * wx0).astype(F) + (x[:, :, y0][..., x1] * wx1).astype(F)
        bot = (x[:, :, y1][..., x0] * wx0).astype(F) + (x[:, :, y1][..., x1] * wx1).astype(F)
        v = ((top * wy0[:, None]).astype(F) + (bot * wy1[:, None]).astype(F)).astype(F)
        return ((v * F(1)).astype(F) + (v * F(0)).astype(F)).astype(F)


def intrinsics_resize(k: np.ndarray, f) -> np.ndarray:
    k = torch.from_numpy(k.copy())  # (:281-285: torch float32 tensor with Python float factors)
    k[0, 0, :] = k[0, 0, :] * f[1]
    k[1, 1, :] = k[1, 1, :] * f[0]
    k[0, 2, :] = (k[0, 2, :] + 0.5) * f[1] - 0.5
    k[1, 2, :] = (k[1, 2, :] + 0.5) * f[0] - 0.5
    return k.numpy()


def restate(raw: Dict[str, np.ndarray], crop_size=(16, 224, 224), track_2d_traj_per_sample: int = 128, center_crop: bool = False,
            start_crop_time: bool = False, resize_size=None, resize_mode: Optional[dict] = None, estimation_directions=(1, -1),
            length_mutiply_of: int = 8, track_2d_querry_sampling_version=None, track_2d_querry_sampling_spacing: float = 0.02,
            remove_queries_outside_bounds: bool = True, scale_queries_on_resize: bool = False, strings: Optional[dict] = None
            ) -> Dict[str, object]:
    """ds[0] of an L4PDataset over ``raw`` with these constructor arguments.  The caller seeds torch (torch.manual_seed) first.
    Also returns "_offsets" = (t0, i0, j0) and "_kept" (indices of the kept queries, or None)."""
    x = {k: np.array(v) for k, v in raw.items()}
    T0, H, W = x["rgb_b3thw"].shape[1:]
    if "intrinsics_b44t" not in x:
        x["intrinsics_b44t"] = np.repeat(np.eye(4, dtype=F)[:, :, None], T0, axis=2)
    if crop_size is None:
        crop_size = (int(math.ceil(max(T0, 16) / length_mutiply_of) * length_mutiply_of), 224, 224)
    Tn, Hn, Wn = crop_size
    x = pad(x, Tn)
    # resize
    modes = {k: "nearest" for k in DENSE}
    modes["rgb_b3thw"] = "trilinear"
    modes.update(resize_mode or {})
    if resize_size is not None:
        rh, rw = (resize_size, resize_size) if isinstance(resize_size, int) else resize_size
        f = (rh / H, rw / W)
        if not (f[0] == 1.0 and f[1] == 1.0):
            for k in list(x):
                if k in DENSE:
                    if modes[k] == "nearest":
                        x[k] = x[k][:, :, torch_nearest_index(H, rh)][..., torch_nearest_index(W, rw)]
                    else:
                        x[k] = bilinear(x[k].astype(F), rh, rw)
                    if k in ("flow_2d_backward_b2thw", "flow_2d_forward_b2thw"):
                        x[k] = np.stack([x[k][0] * F(f[1]), x[k][1] * F(f[0])]).astype(F)
                elif k == "track_2d_traj_bn2t":
                    x[k] = np.stack([x[k][:, 0] * F(f[1]), x[k][:, 1] * F(f[0])], axis=1).astype(F)
                elif k == "intrinsics_b44t":
                    x[k] = intrinsics_resize(x[k], f)
                elif k in QUERY:
                    if not scale_queries_on_resize:
                        raise NotImplementedError(k)
                    if k == "track_2d_pointquerries_bn3":
                        q = x[k]
                        x[k] = np.stack([q[:, 0], q[:, 1] * F(f[1]), q[:, 2] * F(f[0])], axis=1).astype(F)
    # crop
    T, Hc, Wc = x["rgb_b3thw"].shape[1:]
    diff = (T - Tn, Hc - Hn, Wc - Wn)
    assert min(diff) >= 0, f"Cropping Error: diff_shape {list(diff)}"
    offsets, kept = (0, 0, 0), None
    if any(diff):
        t0 = 0 if diff[0] <= 0 else int(torch.randint(0, diff[0], (1,))[0])
        if start_crop_time:
            t0 = 0
        if center_crop:
            i0, j0 = int(diff[1] * 0.5), int(diff[2] * 0.5)
        else:
            i0 = 0 if diff[1] <= 0 else int(torch.randint(0, diff[1], (1,))[0])
            j0 = 0 if diff[2] <= 0 else int(torch.randint(0, diff[2], (1,))[0])
        offsets = (t0, i0, j0)
        for k in list(x):
            if k in DENSE:
                x[k] = x[k][:, t0:t0 + Tn, i0:i0 + Hn, j0:j0 + Wn]
            elif k in TRACKS_T + CAMERAS:
                x[k] = x[k][..., t0:t0 + Tn]
        if "track_2d_pointquerries_bn3" in x and remove_queries_outside_bounds:
            q = x["track_2d_pointquerries_bn3"]
            keep = (q[:, 0] > F(t0)) & (q[:, 0] < F(t0 + Tn)) & (q[:, 1] > F(j0)) & (q[:, 1] < F(j0 + Wn)) & (q[:, 2] > F(i0)) & \
                   (q[:, 2] < F(i0 + Hn))
            kept = np.nonzero(keep)[0]
            for k in TRACKS_T + QUERY:
                if k in x:
                    x[k] = x[k][keep]
        if "track_2d_traj_bn2t" in x:
            tr = x["track_2d_traj_bn2t"]
            tr = np.stack([tr[:, 0] - F(j0), tr[:, 1] - F(i0)], axis=1).astype(F)
            x["track_2d_traj_bn2t"] = tr
            out_of_view = (tr[:, 0] >= F(Wn)) | (tr[:, 0] < 0) | (tr[:, 1] >= F(Hn)) | (tr[:, 1] < 0)
            x["track_2d_vis_bn1t"] = x["track_2d_vis_bn1t"] & ~out_of_view[:, None]
        k = x["intrinsics_b44t"].copy()
        k[0, 2] = k[0, 2] - F(j0)
        k[1, 2] = k[1, 2] - F(i0)
        x["intrinsics_b44t"] = k
        if "track_2d_pointquerries_bn3" in x:
            x["track_2d_pointquerries_bn3"] = (x["track_2d_pointquerries_bn3"] - np.array([t0, j0, i0], dtype=F)).astype(F)
    # queries / dummy ground truth
    if "track_2d_pointquerries_bn3" not in x:
        if track_2d_querry_sampling_version == "uniform":
            q = po.grid_queries(track_2d_querry_sampling_spacing, Tn, Hn, Wn)
            n = q.shape[0]
        elif track_2d_querry_sampling_version is None:
            n = track_2d_traj_per_sample
            q = torch.rand((n, 3)).numpy().astype(F)
            q[:, 0] = 0
            for i, size in enumerate((Tn, Wn, Hn)):
                q[:, i] = torch.round(torch.from_numpy(q[:, i] * F(size - 1))).numpy() + F(0.5)
        else:
            raise NotImplementedError(track_2d_querry_sampling_version)
        x["track_2d_traj_bn2t"] = np.zeros((n, 2, Tn), dtype=F)
        x["track_2d_vis_bn1t"] = np.zeros((n, 1, Tn), dtype=bool)
        x["track_2d_depth_bn1t"] = np.ones((n, 1, Tn), dtype=F)
        x["track_2d_valid_bn1t"] = np.zeros((n, 1, Tn), dtype=bool)
        x["track_2d_pointquerries_bn3"] = np.asarray(q, dtype=F)
        x["track_2d_pointlabels_bn"] = np.ones(n, dtype=F)
    # causal fix
    if len(estimation_directions) != 2:
        time = np.arange(Tn, dtype=F)[None, :] + F(0.5)
        qt = x["track_2d_pointquerries_bn3"][:, 0][:, None]
        ok = time >= qt if estimation_directions[0] == 1 else time <= qt
        x["track_2d_valid_bn1t"] = x["track_2d_valid_bn1t"] & ok[:, None, :]
    with np.errstate(invalid="ignore"):
        x["rgb_b3thw"] = ((x["rgb_b3thw"].astype(F) - MEAN[:, None, None, None]) / STD[:, None, None, None]).astype(F)
    x["rgb_mean_b3111"] = MEAN[:, None, None, None]
    x["rgb_std_b3111"] = STD[:, None, None, None]
    out = {k: np.ascontiguousarray(v) for k, v in x.items()}
    out.update(strings or {})
    out["ori_video_len"] = T0
    out["_offsets"] = offsets
    out["_kept"] = kept
    return out


# ---- fixture access -----------------------------------------------------------------------------------------------------

FULL_LIMIT = 4096  # tensors with more elements are stored as a SHA-256 of their bytes plus sampled values


def bits(a: np.ndarray) -> np.ndarray:
    """Float arrays as uint32 (nan and inf entries count in an equality test), everything else as it is."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a

TOL = 2e-6  # tests/test_preprocess_gpu.py: the bilinear resize against ATen's own arithmetic


def load_golden() -> Dict[str, np.ndarray]:
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_dataset.npz")
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def compare_with_fixture(golden, name, got, exact_only=False):
    """``got`` (key -> numpy array / value) against the reference's sample of case ``name``: keys, dtypes, shapes; bit equality for
    everything gathered or computed with one rounding per operation; TOL * max(1, max |finite value|) for the trilinear fields."""
    case = CASES[name]
    keys = [str(k) for k in golden[name + ".keys"]]
    assert sorted(k for k in got if not k.startswith("_")) == keys
    modes = {k: "nearest" for k in DENSE}
    modes["rgb_b3thw"] = "trilinear"
    modes.update(case["ctor"].get("resize_mode", {}))
    resized = case["ctor"].get("resize_size") is not None
    for k, dt in zip(keys, golden[name + ".dtypes"]):
        v = got[k]
        if f"{name}.{k}.shape" not in golden:  # strings, ori_video_len
            assert type(v).__name__ == str(dt) and np.array(v) == golden[f"{name}.{k}"], k
            continue
        assert str(torch.from_numpy(v).dtype) == str(dt), (k, v.dtype, dt)
        assert list(v.shape) == golden[f"{name}.{k}.shape"].tolist(), k
        interpolated = resized and k in DENSE and modes[k] == "trilinear"
        if f"{name}.{k}" in golden:
            want, mine = golden[f"{name}.{k}"], v
        else:
            idx = golden[f"{name}.{k}.idx"]
            want, mine = golden[f"{name}.{k}.val"], v.reshape(-1)[idx]
            if not interpolated:
                assert hashlib.sha256(np.ascontiguousarray(v).tobytes()).digest() == golden[f"{name}.{k}.sha256"].tobytes(), k
        if not interpolated:
            assert np.array_equal(bits(mine), bits(want)), k
        elif not exact_only:
            fin = np.isfinite(want)
            assert np.array_equal(fin, np.isfinite(mine)), k
            assert np.array_equal(bits(mine[~fin]), bits(want[~fin])) or np.array_equal(np.isnan(mine[~fin]), np.isnan(want[~fin])), k
            bound = TOL * max(1.0, float(np.abs(want[fin]).max()))
            err = float(np.abs(mine[fin] - want[fin]).max())
            print(f"{name}.{k}: max |err| {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (k, err, bound)


def make_dataset(raw, name="clip", **ctor):
    from l4p_amd.data.l4p_dataset_mini import L4PData, L4PDataset

    class Synthetic(L4PDataset):
        def __len__(self):
            return 1

        def getitem_helper(self, index):
            return L4PData(dataset_name="synthetic", seq_name=name, **self.tensors)

    ds = Synthetic(**ctor)
    ds.tensors = {k: torch.from_numpy(np.array(v)) for k, v in raw.items()}
    return ds
