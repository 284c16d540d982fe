"""Dense DPT heads on the MI355X engine — host mirror of l4p/models/task_heads/dense_heads.py.

Same class names, constructor arguments, ``forward`` / ``forward_windowed`` signatures and output keys
as the reference; the decoder runs in libl4p_hip.so as one native call per head (l4p_dpt_forward:
channels-last tensors, implicit-GEMM 3x3x3 convs, ConvTranspose-as-GEMM, fused ReLU / bias / skip
epilogues).  csrc/api_dpt.hip is the one statement of that graph.

One algebraic re-ordering versus the reference graph (csrc/api_dpt.hip, run()): FeatureFusionBlock's
``out_conv`` (a 1x1x1 conv) is applied BEFORE the trilinear up-sampling instead of after it
(dpt_block.py:229-237).  Both are linear and the interpolation weights sum to one, so the result is
identical up to float rounding, while the conv runs on 2-8x fewer voxels.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from ...weights import ModelCfg, actpost_of, fusion_of
from ..aligner import LstSqAffineAligner, LinearAligner, WindowOverlapAligner


class _Runtime:
    """What a head needs at run time; attached by L4P_VideoMAE once weights are loaded."""

    def __init__(self, cfg: ModelCfg, weights, dtype: int):
        self.cfg, self.weights, self.dtype = cfg, weights, dtype


class VideoMAEFlowDPTHead(torch.nn.Module):
    """2D optical-flow DPT head (dense_heads.py:20-143)."""

    def __init__(
        self,
        task_name: str,
        out_nchan: int = 2,
        depth: int = 40,
        embed_dim: int = 1408,
        hooks_idx: Optional[List[int]] = None,
        actpost_scale_factors: Tuple[Tuple, ...] = ((1, 2, 2), (1, 1, 1), (0, 0, 0), (-1, -1, -1)),
        fusion_scale_factors: Tuple[Tuple, ...] = ((1, 2, 2), (1, 2, 2), (2, 2, 2), (2, 2, 2)),
        output_size: Optional[Tuple[int, int, int]] = None,
        overlap_aligner_type=None,
        aligner_kwargs: Dict = {},
    ) -> None:
        super().__init__()
        self.task_name = task_name
        self.out_nchan = out_nchan
        self.depth, self.embed_dim = depth, embed_dim
        self.hooks_idx = list(hooks_idx) if hooks_idx is not None else [depth * 2 // 5, depth * 3 // 5, depth * 4 // 5, depth]
        self.actpost_scale_factors = actpost_scale_factors
        self.fusion_scale_factors = fusion_scale_factors
        self.output_size = output_size
        self.overlap_aligner_type = overlap_aligner_type
        self.aligner_kwargs = aligner_kwargs
        self.task_suffix = f"b{out_nchan}thw"
        self._rt: Optional[_Runtime] = None
        self._engine_task = ""  # key under which the ModuleDict holds this head (== packed weight prefix)
        self._post_exp = False

    # -- engine plumbing -------------------------------------------------------------------------
    def required_taps(self) -> List[int]:
        return list(self.hooks_idx)

    def _decode(self, enc_features_bpc_list, img_info) -> torch.Tensor:
        pre = getattr(enc_features_bpc_list, "decoded", None)
        if pre is not None and self._engine_task in pre:
            return pre[self._engine_task]  # window decoded earlier / on another rank (parallel.DecodedWindow)
        eng = getattr(self._rt, "engine", None)
        if eng is None:
            raise RuntimeError(f"head '{self.task_name}' has no weights: call load_state_dict on the model first")
        hooks = [enc_features_bpc_list.T(h) for h in self.hooks_idx]
        out_ch = self._rt.weights[f"dpt.{self._engine_task}.out.w"].shape[0]
        osz = tuple(img_info) if self.output_size is None else tuple(self.output_size)
        return eng.dpt_forward(self._engine_task, hooks, out_ch, actpost_of(self._engine_task), fusion_of(self._engine_task),
                               osz, self._post_exp)

    # -- reference API ---------------------------------------------------------------------------
    def forward(self, enc_features_bpc_list, img_info: Tuple[int, int, int] = (16, 224, 224), **kwargs) -> Dict[str, torch.Tensor]:
        task_out = self._decode(enc_features_bpc_list, img_info)
        return {f"{self.task_name}_est_{self.task_suffix}": task_out[:, : self.out_nchan]}

    def forward_windowed(self, enc_features_bpc_2dlist, img_info: Tuple[int, int, int] = (16, 224, 224),
                         time_strides: Optional[torch.Tensor] = None, intrinsics_b44t: Optional[torch.Tensor] = None,
                         **kwargs) -> Dict[str, torch.Tensor]:
        """Per-window decode + stitching (dense_heads.py:76-143)."""
        if time_strides is None:
            return self.forward(enc_features_bpc_2dlist[0], img_info=img_info, intrinsics_b44t=intrinsics_b44t, **kwargs)
        window_size = img_info[0] if self.output_size is None else self.output_size[0]
        T = int(time_strides[-1]) + window_size
        key = f"{self.task_name}_est_{self.task_suffix}"
        est = None
        for win_id in range(len(time_strides)):
            kwargs["win_id"] = win_id
            st = int(time_strides[win_id])
            cur = self.forward(
                enc_features_bpc_2dlist[win_id], img_info=img_info,
                intrinsics_b44t=None if intrinsics_b44t is None else intrinsics_b44t[..., st:st + window_size], **kwargs)
            out = cur[key]
            if est is None:
                shp = list(out.shape)
                shp[2] = T
                est = torch.zeros(*shp, dtype=out.dtype, device=out.device)
            if win_id > 0 and self.overlap_aligner_type is not None:
                aligner = self.overlap_aligner_type(**self.aligner_kwargs)
                ov = int(time_strides[win_id - 1]) + window_size - st
                aligner.solve(out[:, :, :ov], est[:, :, st:st + ov],
                              None if intrinsics_b44t is None else intrinsics_b44t[..., st:st + ov], img_info)
                out = aligner.apply(out)
            if self.task_name == "flow_2d_backward" and win_id > 0:
                est[:, :, st + 1:st + window_size] = out[:, :, 1:]  # first frame of a later window is invalid
            else:
                est[:, :, st:st + window_size] = out
        return {key: est}


class VideoMAEDepthDPTHead(VideoMAEFlowDPTHead):
    """Depth DPT head (dense_heads.py:146-182): exp() on the decoder output, LstSq/linear seam aligner."""

    def __init__(self, task_name: str, out_nchan: int = 1, depth: int = 40, embed_dim: int = 1408,
                 depth_fn: str = "linear", hooks_idx: Optional[List[int]] = None,
                 align_window_overlap_fn: Optional[str] = None, align_type: str = "affine") -> None:
        if align_type not in ("affine", "linear"):
            raise ValueError(f"align_type={align_type!r}: expected 'affine' or 'linear'")
        super().__init__(task_name, out_nchan, depth, embed_dim, hooks_idx,
                         overlap_aligner_type=LstSqAffineAligner if align_type == "affine" else LinearAligner,
                         aligner_kwargs=dict(pre_post_fn=align_window_overlap_fn))
        if depth_fn not in ("exp", "linear"):
            raise NotImplementedError(f"depth_fn={depth_fn!r}: the engine fuses 'exp' or 'linear' into the output kernel")
        self.depth_fn = depth_fn
        self._post_exp = depth_fn == "exp"


class VideoMAEDynMaskDPTHead(VideoMAEFlowDPTHead):
    """Dynamic-mask DPT head (dense_heads.py:185-217)."""

    def __init__(self, task_name: str, out_nchan: int = 1, depth: int = 40, embed_dim: int = 1408,
                 apply_fn: str = "linear", hooks_idx: Optional[List[int]] = None) -> None:
        super().__init__(task_name, out_nchan, depth, embed_dim, hooks_idx, overlap_aligner_type=None)
        if apply_fn != "linear":
            raise NotImplementedError(f"apply_fn={apply_fn!r} is not used by configs/model.yaml")
        self.apply_fn = apply_fn

    def forward(self, enc_features_bpc_list, img_info=(16, 224, 224), **kwargs):
        return {f"{self.task_name}_est_{self.task_suffix}": self._decode(enc_features_bpc_list, img_info)}


class VideoMAETraj3DDPTHead(VideoMAEFlowDPTHead):
    """Ray-map head -> camera poses (dense_heads.py:257-352)."""

    def __init__(self, task_name: str, depth: int = 40, embed_dim: int = 1408, hooks_idx: Optional[List[int]] = None,
                 actpost_scale_factors=((1, 0, 0), (1, 0, 0), (0, 0, 0), (-1, -1, -1)),
                 fusion_scale_factors=((1, 1, 1), (1, 1, 1), (2, 1, 1), (2, 2, 2)),
                 output_size: Optional[Tuple[int, int, int]] = (16, 16, 16), use_intrinsics: bool = True,
                 fixed_intrinsics: bool = False) -> None:
        super().__init__(task_name, 6, depth, embed_dim, hooks_idx, actpost_scale_factors, fusion_scale_factors,
                         output_size)
        self.task_suffix = "b16t"
        self.use_intrinsics = use_intrinsics
        self.fixed_intrinsics = fixed_intrinsics
        self.first_window_intrinsics_b44t = None

    def forward(self, enc_features_bpc_list, img_info=(16, 224, 224), intrinsics_b44t: Optional[torch.Tensor] = None,
                **kwargs) -> Dict[str, torch.Tensor]:
        from ...utils.geometry_utils import intrinsics_from_rays, poses_from_rays

        T, H, W = img_info
        rays = self._decode(enc_features_bpc_list, img_info)  # float [B,6,16,16,16]
        key = f"{self.task_name}_est_{self.task_suffix}"
        if self.use_intrinsics:
            if intrinsics_b44t is None:
                raise ValueError("intrinsics_b44t is required when use_intrinsics=True")
            return {key: poses_from_rays(rays, intrinsics_b44t.to(rays.device, torch.float32), H, W)}
        if not self.fixed_intrinsics:
            # per-frame intrinsics and extrinsics (dense_heads.py:336-344): every frame's own K, rotation from its RQ step
            from ...utils.geometry_utils import cameras_from_rays_variable_intrinsics

            pose, K_est = cameras_from_rays_variable_intrinsics(rays, H, W, reproj_threshold=0.2)
            return {key: pose, f"{self.task_name}_intrinsics_est_{self.task_suffix}": K_est.reshape(K_est.shape[0], 16, T)}
        # fixed intrinsics, estimated once on the first window (dense_heads.py:303-334)
        assert "win_id" in kwargs, "win_id is required when setting fixed intrinsics as True"
        if kwargs["win_id"] == 0:
            self.first_window_intrinsics_b44t = None
        if self.first_window_intrinsics_b44t is None:
            K_est = intrinsics_from_rays(rays, H, W, reproj_threshold=0.2)  # [B,4,4,T], first frame, pixel units
            pose = poses_from_rays(rays, K_est, H, W)
            self.first_window_intrinsics_b44t = K_est.clone()
        else:
            # as the reference: later windows rotate with the INPUT intrinsics (dense_heads.py:327-333) and report the
            # first window's estimate
            if intrinsics_b44t is None:
                raise ValueError("intrinsics_b44t is required for windows after the first one")
            pose = poses_from_rays(rays, intrinsics_b44t.to(rays.device, torch.float32), H, W)
            K_est = self.first_window_intrinsics_b44t.clone()
        return {key: pose, f"{self.task_name}_intrinsics_est_{self.task_suffix}": K_est.reshape(K_est.shape[0], 16, T)}


def joint_windowed_estimation(task_names: List[str], task_heads: torch.nn.ModuleDict, enc_features_bpc_2dlist,
                              time_strides: Optional[torch.Tensor] = None, intrinsics_b44t: Optional[torch.Tensor] = None,
                              img_info: Tuple[int, int, int] = (16, 224, 224), **kwargs) -> Dict[str, torch.Tensor]:
    """Joint depth + camera estimation over sliding windows (dense_heads.py:360-492): per-window heads, then a
    similarity alignment of the overlap point maps (KabaschUmeyama3DAligner) applied to pose and depth."""
    from ..aligner import KabaschUmeyama3DAligner

    out_all: Dict[str, torch.Tensor] = {}
    if time_strides is None:
        for name in task_names:
            out_all.update(task_heads[name].forward(enc_features_bpc_2dlist[0], img_info=img_info,
                                                    intrinsics_b44t=intrinsics_b44t, **kwargs))
        return out_all
    ws = img_info[0]
    T = int(time_strides[-1]) + ws
    est: Dict[str, Optional[torch.Tensor]] = {name: None for name in task_names}
    est["camray_intrinsics_est"] = None
    cam = task_heads["camray"]
    for win_id in range(len(time_strides)):
        st = int(time_strides[win_id])
        kwargs["win_id"] = win_id
        cur: Dict[str, torch.Tensor] = {}
        for name in task_names:
            head = task_heads[name]
            o = head.forward(enc_features_bpc_2dlist[win_id], img_info=img_info,
                             intrinsics_b44t=intrinsics_b44t[..., st:st + ws], **kwargs)
            cur[name] = o[f"{head.task_name}_est_{head.task_suffix}"]
            if name == "camray":
                kkey = f"{head.task_name}_intrinsics_est_{head.task_suffix}"
                # the reference hard-codes batch 1 here (dense_heads.py:421); clips are independent, so B is kept
                cur["camray_intrinsics_est"] = (o[kkey] if kkey in o else
                                                intrinsics_b44t[..., st:st + ws].clone().reshape(-1, 16, ws))
        for k, v in cur.items():
            if est[k] is None:
                shp = list(v.shape)
                shp[2] = T
                est[k] = torch.zeros(*shp, dtype=v.dtype, device=v.device)
        if win_id > 0:
            aligner = KabaschUmeyama3DAligner()
            ov = int(time_strides[win_id - 1]) + ws - st
            pred = {n: cur[n][:, :, :ov] for n in task_names}
            target = {n: est[n][:, :, st:st + ov] for n in task_names}
            pred["camray_intrinsics"] = cur["camray_intrinsics_est"][:, :, :ov].reshape(-1, 4, 4, ov).clone()
            target["camray_intrinsics"] = est["camray_intrinsics_est"][:, :, st:st + ov].reshape(-1, 4, 4, ov)
            aligner.solve(pred, target, img_info)
            cur = aligner.apply(cur)
        for k, v in cur.items():
            est[k][:, :, st:st + ws] = v
    for name in task_names:
        head = task_heads[name]
        out_all[f"{head.task_name}_est_{head.task_suffix}"] = est[name]
    out_all[f"{cam.task_name}_intrinsics_est_{cam.task_suffix}"] = est["camray_intrinsics_est"]
    return out_all
