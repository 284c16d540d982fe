"""Generate tests/golden/datasets.npz (+ .json provenance) from the REAL reference dataset classes (runs only where the
reference checkout is importable, --ref).

  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_datasets.py --ref DIR

The reference's `l4p.data.davis.DavisDataset` and `l4p.data.dycheck_dataset.DycheckDataset` are imported and their own
`__getitem__` is run on seeded directory trees written to a temporary directory (l4p_amd.data.synthetic.write_davis_tree /
write_dycheck_tree; the ".jpg" frames hold PNG bytes, so the decoded frames are exactly the seeded arrays on any libjpeg).
Modules the image lacks are stubbed at import time, as in tools/gen_golden_preprocess.py:
  * mediapy        — imported by davis.py:12, only used by a helper the dataset never calls;
  * torchvision.transforms.functional — only `to_tensor`: uint8 HWC (or HW for "P" / "L" images) -> float32 CHW / 255;
  * kornia.morphology.erosion — NOT installed and its source is not available: the stand-in restates its definition for the
    default border_type="geodesic" (out-of-image neighbours never lower the minimum).  Unpinned by construction.
PIL and torch are the real ones.  Only data is written: case parameters, the small tensors in full, the first mask frame
bit-packed, a SHA-256 of the whole mask tensor and sampled RGB values.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import tempfile
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from l4p_amd.data.synthetic import write_davis_tree, write_dycheck_tree
from tests import datasets_restate as dr
from tests.golden_utils import sample_indices


def _to_tensor(pic):
    a = np.asarray(pic)
    if a.dtype == bool:
        a = a.astype(np.uint8) * 255
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(a).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def _erosion(x, kernel):
    assert tuple(kernel.shape) == (3, 3) and bool((kernel == 1).all())
    return -torch.nn.functional.max_pool2d(-x, 3, stride=1, padding=1)  # the pool pads with -inf: geodesic border


def install_stubs(ref):
    media = types.ModuleType("mediapy")
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")
    tvf.to_tensor = _to_tensor
    tv.transforms, tvt.functional = tvt, tvf
    kornia = types.ModuleType("kornia")
    km = types.ModuleType("kornia.morphology")
    km.erosion = _erosion
    kornia.morphology = km
    sys.modules.update({"mediapy": media, "torchvision": tv, "torchvision.transforms": tvt,
                        "torchvision.transforms.functional": tvf, "kornia": kornia, "kornia.morphology": km})
    sys.path.insert(0, ref)


def record(out, name, s):
    rgb = s["rgb_b3thw"].numpy()
    idx = sample_indices(rgb.size, 2048).numpy()
    out[name + ".rgb_shape"] = np.array(rgb.shape)
    out[name + ".rgb_idx"] = idx
    out[name + ".rgb_val"] = rgb.reshape(-1)[idx]
    out[name + ".intrinsics_b44t"] = s["intrinsics_b44t"].numpy()
    out[name + ".queries"] = s["track_2d_pointquerries_bn3"].numpy()
    out[name + ".ori_video_len"] = np.array(s["ori_video_len"])
    out[name + ".seq_name"] = np.array(s["seq_name"])
    out[name + ".keys"] = np.array(sorted(s.keys()))
    out[name + ".dtypes"] = np.array([str(s[k].dtype) if torch.is_tensor(s[k]) else type(s[k]).__name__ for k in sorted(s.keys())])
    if "extrinsics_b44t" in s:
        out[name + ".extrinsics_b44t"] = s["extrinsics_b44t"].numpy()
    if "instanceseg_b1thw" in s:
        m = s["instanceseg_b1thw"].numpy()
        assert set(np.unique(m)) <= {0.0, 1.0}
        out[name + ".mask_shape"] = np.array(m.shape)
        out[name + ".mask_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(m).tobytes()).digest(), dtype=np.uint8)
        out[name + ".mask_frame0_bits"] = np.packbits(m[0, 0].astype(np.uint8))
        out[name + ".mask_sum"] = np.array(m.sum(dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (NVlabs/L4P)")
    install_stubs(ap.parse_args().ref)
    import PIL

    from l4p.data.davis import DavisDataset
    from l4p.data.dycheck_dataset import DycheckDataset

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, c in dr.DAVIS_CASES.items():
            frames, masks = dr.case_inputs(name)
            root = write_davis_tree(os.path.join(tmp, "davis_" + name), name, frames, masks, c["mode"])
            ds = DavisDataset(data_root=root, stride=c["stride"], crop_size=c["crop_size"], resize_size=tuple(c["resize_size"]),
                              estimation_directions=[1], track_2d_querry_sampling_spacing=c["spacing"])
            assert len(ds) == 1
            s = ds[0]
            record(out, name, s)
            o = dr.davis_sample(frames, dr.annotation_arrays(masks, c["mode"]), c["mode"], c["crop_size"], tuple(c["resize_size"]),
                                c["stride"], c["spacing"])
            err = float(np.abs(o["rgb_b3thw"] - s["rgb_b3thw"].numpy()).max())
            assert err <= 2e-6, (name, err)
            for k in ("instanceseg_b1thw", "intrinsics_b44t", "track_2d_pointquerries_bn3"):
                assert np.array_equal(o[k], s[k].numpy()), (name, k)
            out[name + ".restatement_max_abs_err"] = np.array(err)
            print(f"{name}: mask sum {float(out[name + '.mask_sum']):.0f}  queries {out[name + '.queries'].shape[0]} of "
                  f"{dr.seg_cells(c['spacing']).shape[0]}  rgb restatement max|err| {err:.2e}")
        for name, c in dr.DYCHECK_CASES.items():
            frames, _ = dr.case_inputs(name)
            root = write_dycheck_tree(os.path.join(tmp, "dycheck_" + name), name, frames, c["calibration"])
            ds = DycheckDataset(data_root=root, stride=c["stride"], crop_size=c["crop_size"], resize_size=tuple(c["resize_size"]),
                                estimation_directions=[1], track_2d_querry_sampling_spacing=c["spacing"])
            assert len(ds) == 1
            s = ds[0]
            record(out, name, s)
            o = dr.dycheck_sample(frames, c["calibration"], c["crop_size"], tuple(c["resize_size"]), c["stride"], c["spacing"])
            err = float(np.abs(o["rgb_b3thw"] - s["rgb_b3thw"].numpy()).max())
            assert err <= 2e-6, (name, err)
            for k in ("extrinsics_b44t", "intrinsics_b44t", "track_2d_pointquerries_bn3"):
                assert np.array_equal(o[k], s[k].numpy()), (name, k)
            out[name + ".restatement_max_abs_err"] = np.array(err)
            print(f"{name}: K {s['intrinsics_b44t'][:2, :3, 0].tolist()}  rgb restatement max|err| {err:.2e}")
    path = os.path.join(ROOT, "tests", "golden", "datasets.npz")
    np.savez_compressed(path, **out)
    prov = {
        "generator": "tools/gen_golden_datasets.py",
        "source": "the reference's l4p.data.davis.DavisDataset / l4p.data.dycheck_dataset.DycheckDataset, their own __getitem__",
        "pillow": PIL.__version__, "torch": torch.__version__.split("+")[0], "numpy": np.__version__,
        "stand_ins": {
            "mediapy": "empty module (imported by davis.py, not used by the dataset)",
            "torchvision.transforms.functional.to_tensor": "uint8 HWC or HW -> float32 CHW / 255",
            "kornia.morphology.erosion": "NOT the real one (not installed, source unavailable): -max_pool2d(-x, 3, 1, padding=1), i.e. "
                                         "kornia's default border_type='geodesic' - out-of-image neighbours never lower the minimum; "
                                         "unpinned by construction",
        },
        "inputs": "seeded trees: l4p_amd.data.synthetic (synthetic_video / synthetic_masks / write_*_tree); '.jpg' files hold PNG bytes",
        "cases": {"davis": dr.DAVIS_CASES, "dycheck": dr.DYCHECK_CASES},
    }
    with open(path[:-4] + ".json", "w") as f:
        json.dump(prov, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
