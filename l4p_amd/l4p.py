"""L4PLitModule — host mirror of l4p/l4p.py (inference and evaluation surface: forward / step / predict_step / validation_step /
test_step).

Subclasses lightning.LightningModule when lightning is importable (as the reference does), otherwise
torch.nn.Module; either way ``forward(batch, tasks)`` and ``predict_step(batch, batch_idx)`` behave as in
l4p.py:37-39,54-66,107-109, and ``step("val" | "test")`` / ``validation_step`` / ``test_step`` follow l4p.py:68-105: the loss module
if there is one, the metrics module (``l4p.metrics.L4PMetrics``) under inference mode, the ``scalars/{phase}/...`` log kept as
``self.last_log``.  There is no backward pass in this engine: ``step("train")`` raises, and the reference's optimiser hooks
(losses/optimisers are ``None`` in the release) are out of scope.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

try:  # pragma: no cover - lightning is not installed in the build image
    import lightning as L

    _Base = L.LightningModule
except Exception:  # noqa: BLE001
    _Base = torch.nn.Module


class L4PLitModule(_Base):
    def __init__(
        self,
        tasks: List[str],
        l4p_model: torch.nn.Module,
        loss_module: Optional[torch.nn.Module] = None,
        metrics_module: Optional[torch.nn.Module] = None,
        optimizer_opts: Optional[Dict[str, Any]] = None,
        scheduler_opts: Optional[Dict[str, Any]] = None,
        strict_loading: bool = True,
    ):
        super().__init__()
        self.tasks = tasks
        self.l4p_model = l4p_model
        self.loss_module = loss_module
        self.metrics_module = metrics_module
        self.optimizer_opts = optimizer_opts
        self.scheduler_opts = scheduler_opts
        self._strict = strict_loading

    def forward(self, batch, tasks):
        return self.l4p_model.forward(batch, tasks)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Lightning checkpoint layout: every key prefixed with ``l4p_model.`` (l4p.py:27)."""
        return self.l4p_model.load_state_dict(state_dict, strict=strict and self._strict)

    def step(self, phase, batch, batch_idx):
        dev = self.l4p_model.device
        for key in list(batch.keys()):
            if torch.is_tensor(batch[key]):
                batch[key] = batch[key].to(device=dev)
        out = self.forward(batch, self.tasks)
        if phase == "predict":
            return out
        if phase == "train":
            raise NotImplementedError("there is no backward pass in the MI355X engine: only the predict, val and test phases")
        skip = False
        loss, loss_dict, metadata = self.loss_module(batch, out) if self.loss_module is not None else (0, {}, {})
        with torch.inference_mode():
            metrics_dict = {}
            if self.metrics_module is not None:
                metrics_dict, _ = self.metrics_module(batch, out, metadata)
            log = {f"scalars/{phase}/loss": torch.clone(loss).to(torch.float32) if torch.is_tensor(loss) else loss}
            for key in loss_dict.keys():
                log[f"scalars/{phase}/{key}"] = torch.clone(loss_dict[key]).to(torch.float32)
            for key in metrics_dict.keys():
                log[f"scalars/{phase}/{key}"] = torch.clone(metrics_dict[key]).to(torch.float32)
            self.last_log = log
            if _Base is not torch.nn.Module:  # Lightning's logger; without Lightning last_log is the record
                self.log_dict(log)
        return loss, out, skip

    def validation_step(self, batch, batch_idx):
        loss, out, skip = self.step("val", batch, batch_idx)
        return {"loss": loss, "out": out} if not skip else None

    def test_step(self, batch, batch_idx):
        loss, out, skip = self.step("val", batch, batch_idx)  # (the reference logs its test phase under "val", l4p.py:104)
        return {"loss": loss, "out": out} if not skip else None

    def predict_step(self, batch, batch_idx):
        return self.step("predict", batch, batch_idx)
