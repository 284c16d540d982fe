"""Generate tests/golden/gt_dataset.npz (+ .json provenance) from the REAL reference L4PDataset base class (runs only where the
reference checkout is importable, --ref).

  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_gt_dataset.py --ref DIR

The reference's `l4p.data.l4p_dataset_mini.L4PDataset` is imported and subclassed with a `getitem_helper` over
l4p_amd.data.synthetic.synthetic_ground_truth; for every case of tests/gt_dataset_restate.py `torch.manual_seed` is called and the
reference's own `__getitem__` is run on the CPU.  kornia (imported by the module, used only by "uniform_over_seg" sampling, which
no case here selects) is stubbed as in tools/gen_golden_datasets.py.  Only data is written: every output tensor in full, or,
above 4096 elements, its shape, a SHA-256 of its bytes and 2048 sampled values; the strings; the keys and dtypes.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from tests import gt_dataset_restate as gr
from tests.golden_utils import sample_indices


def install_stubs(ref):
    kornia = types.ModuleType("kornia")
    km = types.ModuleType("kornia.morphology")

    def erosion(x, kernel):
        raise NotImplementedError("kornia.morphology.erosion is not installed; no case of this fixture uses it")

    km.erosion = erosion
    kornia.morphology = km
    sys.modules.update({"kornia": kornia, "kornia.morphology": km})
    sys.path.insert(0, ref)


def record(out, name, s):
    keys = sorted(s.keys())
    out[name + ".keys"] = np.array(keys)
    out[name + ".dtypes"] = np.array([str(s[k].dtype) if torch.is_tensor(s[k]) else type(s[k]).__name__ for k in keys])
    for k in keys:
        v = s[k]
        if not torch.is_tensor(v):
            out[f"{name}.{k}"] = np.array(v)
            continue
        a = np.ascontiguousarray(v.numpy())
        out[f"{name}.{k}.shape"] = np.array(a.shape, dtype=np.int64)
        if a.size <= gr.FULL_LIMIT:
            out[f"{name}.{k}"] = a
        else:
            idx = sample_indices(a.size, 2048).numpy()
            out[f"{name}.{k}.sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            out[f"{name}.{k}.idx"] = idx
            out[f"{name}.{k}.val"] = a.reshape(-1)[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (NVlabs/L4P)")
    install_stubs(ap.parse_args().ref)
    from l4p.data.l4p_dataset_mini import L4PData, L4PDataset

    class Synthetic(L4PDataset):
        def __init__(self, raw, name, **kw):
            super().__init__(**kw)
            self.raw, self.name = raw, name

        def __len__(self):
            return 1

        def getitem_helper(self, index):
            return L4PData(dataset_name="synthetic", seq_name=self.name, **{k: torch.from_numpy(v.copy()) for k, v in self.raw.items()})

    out, report = {}, {}
    for name, case in gr.CASES.items():
        raw = gr.case_raw(case)
        ds = Synthetic(raw, name, **case["ctor"])
        torch.manual_seed(case["manual_seed"])
        s = ds[0]
        record(out, name, s)
        torch.manual_seed(case["manual_seed"])
        r = gr.restate(raw, **case["ctor"])
        worst = {}
        for k in s:
            if not torch.is_tensor(s[k]):
                continue
            a, b = s[k].numpy(), r[k]
            assert a.shape == b.shape and a.dtype == b.dtype, (name, k, a.shape, b.shape, a.dtype, b.dtype)
            if not np.array_equal(gr.bits(a), gr.bits(b)):
                fin = np.isfinite(a) & np.isfinite(b)
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin], b[~fin], equal_nan=True), (name, k, "nan / inf differ")
                worst[k] = float(np.abs(a[fin] - b[fin]).max()) if a.dtype == np.float32 else "DIFFERS"
        nq = int(s["track_2d_pointquerries_bn3"].shape[0])
        report[name] = dict(offsets=[int(v) for v in r["_offsets"]], queries=nq, restatement_not_bit_equal=worst)
        out[name + ".offsets"] = np.array(r["_offsets"], dtype=np.int64)
        print(name, report[name])
    path = os.path.join(ROOT, "tests", "golden", "gt_dataset.npz")
    np.savez_compressed(path, **out)
    prov = {
        "generator": "tools/gen_golden_gt_dataset.py",
        "source": "the reference's l4p.data.l4p_dataset_mini.L4PDataset, its own __getitem__ on the CPU",
        "torch": torch.__version__.split("+")[0], "numpy": np.__version__,
        "stand_ins": {"kornia.morphology.erosion": "raises (imported by the module; no case uses uniform_over_seg sampling)"},
        "inputs": "l4p_amd.data.synthetic.synthetic_ground_truth; torch.manual_seed(manual_seed) before ds[0]",
        "cases": gr.CASES,
        "report": report,
    }
    with open(path[:-4] + ".json", "w") as f:
        json.dump(prov, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
