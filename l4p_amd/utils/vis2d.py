"""The demo's 2D result video on the GPU: the reference's generate_video_visualizations (l4p/utils/vis.py:34-104) on the engine's
outputs - RGB, turbo-coloured depth, colour-wheel flow, thresholded motion mask and track trails over the grey video, side by
side - with every stage in csrc/vis2d.hip.

``render_video_panels`` returns device tensors without a host synchronisation; ``generate_video_visualizations`` has the
reference's signature and return value.  The module is not named ``vis``: ``l4p.utils.vis`` (cv2 / mediapy / open3d) stays out
of the engine and ``import l4p.utils.vis`` keeps raising ImportError.

What is the reference's and what is this project's own:

* RGB, depth, flow and mask panels follow the reference operation by operation (f32 where it computes in torch f32, float64 where
  it computes in Python floats or numpy float64: under NumPy 2 promotion ``np.clip(f32 array, np.float64 bound)`` is float64, so
  the whole colour-wheel computation after the clip is).  With no positive depth the reference raises; here ``depth_range`` is
  NaN and the depth panel is all zero.
* The track panel keeps the reference's structure and ordering (trail steps, tracks in height order, addWeighted fades, end
  points last) but cv2's anti-aliased coverage cannot be run or read where this was written: segments and discs follow the
  rules stated at ``l4p_vis_track_raster`` (include/l4p_hip.h).  Tracks are ordered by a stable argsort (ties keep their
  index; the reference's torch.argsort leaves ties unspecified), and a primitive with a non-finite coordinate is skipped (the
  reference raises).
* uint8 output uses the project's own rule min(255, max(0, x * 255 + 0.5)) truncated; mediapy's conversion is not asserted.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from .recon4d import _f32, hsv_table

MASK_THR = 0.85  # vis.py:83
TRACK_VIS_THR = 0.5  # vis.py:92
TRACKS_LEAVE_TRACE = 16  # vis.py:92
MAX_FLOW_MAG = 25.0  # vis.py:73
DEPTH_VIS_RANGE = (0.05, 20.0)  # vis.py:58
FPS = 15  # vis.py:100
PANEL_TASKS = ("depth", "flow_2d_backward", "dyn_mask", "track_2d")

# make_colorwheel() (vis.py:288-335; Baker et al., "A Database and Evaluation Methodology for Optical Flow", ICCV 2007): 55 x 3
_WHEEL_DATA = (
    (255, 0, 0), (255, 17, 0), (255, 34, 0), (255, 51, 0), (255, 68, 0), (255, 85, 0), (255, 102, 0), (255, 119, 0),
    (255, 136, 0), (255, 153, 0), (255, 170, 0), (255, 187, 0), (255, 204, 0), (255, 221, 0), (255, 238, 0), (255, 255, 0),
    (213, 255, 0), (170, 255, 0), (128, 255, 0), (85, 255, 0), (43, 255, 0), (0, 255, 0), (0, 255, 63), (0, 255, 127),
    (0, 255, 191), (0, 255, 255), (0, 232, 255), (0, 209, 255), (0, 186, 255), (0, 163, 255), (0, 140, 255), (0, 116, 255),
    (0, 93, 255), (0, 70, 255), (0, 47, 255), (0, 24, 255), (0, 0, 255), (19, 0, 255), (39, 0, 255), (58, 0, 255),
    (78, 0, 255), (98, 0, 255), (117, 0, 255), (137, 0, 255), (156, 0, 255), (176, 0, 255), (196, 0, 255), (215, 0, 255),
    (235, 0, 255), (255, 0, 255), (255, 0, 213), (255, 0, 170), (255, 0, 128), (255, 0, 85), (255, 0, 43),
)

# matplotlib's "turbo" colormap (Google's Turbo, A. Mikhailov 2019, Apache-2.0): its 256 published entries
_TURBO_DATA = (
    (0.18995, 0.07176, 0.23217), (0.19483, 0.08339, 0.26149), (0.19956, 0.09498, 0.29024), (0.20415, 0.10652, 0.31844),
    (0.2086, 0.11802, 0.34607), (0.21291, 0.12947, 0.37314), (0.21708, 0.14087, 0.39964), (0.22111, 0.15223, 0.42558),
    (0.225, 0.16354, 0.45096), (0.22875, 0.17481, 0.47578), (0.23236, 0.18603, 0.50004), (0.23582, 0.1972, 0.52373),
    (0.23915, 0.20833, 0.54686), (0.24234, 0.21941, 0.56942), (0.24539, 0.23044, 0.59142), (0.2483, 0.24143, 0.61286),
    (0.25107, 0.25237, 0.63374), (0.25369, 0.26327, 0.65406), (0.25618, 0.27412, 0.67381), (0.25853, 0.28492, 0.693),
    (0.26074, 0.29568, 0.71162), (0.2628, 0.30639, 0.72968), (0.26473, 0.31706, 0.74718), (0.26652, 0.32768, 0.76412),
    (0.26816, 0.33825, 0.7805), (0.26967, 0.34878, 0.79631), (0.27103, 0.35926, 0.81156), (0.27226, 0.3697, 0.82624),
    (0.27334, 0.38008, 0.84037), (0.27429, 0.39043, 0.85393), (0.27509, 0.40072, 0.86692), (0.27576, 0.41097, 0.87936),
    (0.27628, 0.42118, 0.89123), (0.27667, 0.43134, 0.90254), (0.27691, 0.44145, 0.91328), (0.27701, 0.45152, 0.92347),
    (0.27698, 0.46153, 0.93309), (0.2768, 0.47151, 0.94214), (0.27648, 0.48144, 0.95064), (0.27603, 0.49132, 0.95857),
    (0.27543, 0.50115, 0.96594), (0.27469, 0.51094, 0.97275), (0.27381, 0.52069, 0.97899), (0.27273, 0.5304, 0.98461),
    (0.27106, 0.54015, 0.9893), (0.26878, 0.54995, 0.99303), (0.26592, 0.55979, 0.99583), (0.26252, 0.56967, 0.99773),
    (0.25862, 0.57958, 0.99876), (0.25425, 0.5895, 0.99896), (0.24946, 0.59943, 0.99835), (0.24427, 0.60937, 0.99697),
    (0.23874, 0.61931, 0.99485), (0.23288, 0.62923, 0.99202), (0.22676, 0.63913, 0.98851), (0.22039, 0.64901, 0.98436),
    (0.21382, 0.65886, 0.97959), (0.20708, 0.66866, 0.97423), (0.20021, 0.67842, 0.96833), (0.19326, 0.68812, 0.9619),
    (0.18625, 0.69775, 0.95498), (0.17923, 0.70732, 0.94761), (0.17223, 0.7168, 0.93981), (0.16529, 0.7262, 0.93161),
    (0.15844, 0.73551, 0.92305), (0.15173, 0.74472, 0.91416), (0.14519, 0.75381, 0.90496), (0.13886, 0.76279, 0.8955),
    (0.13278, 0.77165, 0.8858), (0.12698, 0.78037, 0.8759), (0.12151, 0.78896, 0.86581), (0.11639, 0.7974, 0.85559),
    (0.11167, 0.80569, 0.84525), (0.10738, 0.81381, 0.83484), (0.10357, 0.82177, 0.82437), (0.10026, 0.82955, 0.81389),
    (0.0975, 0.83714, 0.80342), (0.09532, 0.84455, 0.79299), (0.09377, 0.85175, 0.78264), (0.09287, 0.85875, 0.7724),
    (0.09267, 0.86554, 0.7623), (0.0932, 0.87211, 0.75237), (0.09451, 0.87844, 0.74265), (0.09662, 0.88454, 0.73316),
    (0.09958, 0.8904, 0.72393), (0.10342, 0.896, 0.715), (0.10815, 0.90142, 0.70599), (0.11374, 0.90673, 0.69651),
    (0.12014, 0.91193, 0.6866), (0.12733, 0.91701, 0.67627), (0.13526, 0.92197, 0.66556), (0.14391, 0.9268, 0.65448),
    (0.15323, 0.93151, 0.64308), (0.16319, 0.93609, 0.63137), (0.17377, 0.94053, 0.61938), (0.18491, 0.94484, 0.60713),
    (0.19659, 0.94901, 0.59466), (0.20877, 0.95304, 0.58199), (0.22142, 0.95692, 0.56914), (0.23449, 0.96065, 0.55614),
    (0.24797, 0.96423, 0.54303), (0.2618, 0.96765, 0.52981), (0.27597, 0.97092, 0.51653), (0.29042, 0.97403, 0.50321),
    (0.30513, 0.97697, 0.48987), (0.32006, 0.97974, 0.47654), (0.33517, 0.98234, 0.46325), (0.35043, 0.98477, 0.45002),
    (0.36581, 0.98702, 0.43688), (0.38127, 0.98909, 0.42386), (0.39678, 0.99098, 0.41098), (0.41229, 0.99268, 0.39826),
    (0.42778, 0.99419, 0.38575), (0.44321, 0.99551, 0.37345), (0.45854, 0.99663, 0.3614), (0.47375, 0.99755, 0.34963),
    (0.48879, 0.99828, 0.33816), (0.50362, 0.99879, 0.32701), (0.51822, 0.9991, 0.31622), (0.53255, 0.99919, 0.30581),
    (0.54658, 0.99907, 0.29581), (0.56026, 0.99873, 0.28623), (0.57357, 0.99817, 0.27712), (0.58646, 0.99739, 0.26849),
    (0.59891, 0.99638, 0.26038), (0.61088, 0.99514, 0.2528), (0.62233, 0.99366, 0.24579), (0.63323, 0.99195, 0.23937),
    (0.64362, 0.98999, 0.23356), (0.65394, 0.98775, 0.22835), (0.66428, 0.98524, 0.2237), (0.67462, 0.98246, 0.2196),
    (0.68494, 0.97941, 0.21602), (0.69525, 0.9761, 0.21294), (0.70553, 0.97255, 0.21032), (0.71577, 0.96875, 0.20815),
    (0.72596, 0.9647, 0.2064), (0.7361, 0.96043, 0.20504), (0.74617, 0.95593, 0.20406), (0.75617, 0.95121, 0.20343),
    (0.76608, 0.94627, 0.20311), (0.77591, 0.94113, 0.2031), (0.78563, 0.93579, 0.20336), (0.79524, 0.93025, 0.20386),
    (0.80473, 0.92452, 0.20459), (0.8141, 0.91861, 0.20552), (0.82333, 0.91253, 0.20663), (0.83241, 0.90627, 0.20788),
    (0.84133, 0.89986, 0.20926), (0.8501, 0.89328, 0.21074), (0.85868, 0.88655, 0.2123), (0.86709, 0.87968, 0.21391),
    (0.8753, 0.87267, 0.21555), (0.88331, 0.86553, 0.21719), (0.89112, 0.85826, 0.2188), (0.8987, 0.85087, 0.22038),
    (0.90605, 0.84337, 0.22188), (0.91317, 0.83576, 0.22328), (0.92004, 0.82806, 0.22456), (0.92666, 0.82025, 0.2257),
    (0.93301, 0.81236, 0.22667), (0.93909, 0.80439, 0.22744), (0.94489, 0.79634, 0.228), (0.95039, 0.78823, 0.22831),
    (0.9556, 0.78005, 0.22836), (0.96049, 0.77181, 0.22811), (0.96507, 0.76352, 0.22754), (0.96931, 0.75519, 0.22663),
    (0.97323, 0.74682, 0.22536), (0.97679, 0.73842, 0.22369), (0.98, 0.73, 0.22161), (0.98289, 0.7214, 0.21918),
    (0.98549, 0.7125, 0.2165), (0.98781, 0.7033, 0.21358), (0.98986, 0.69382, 0.21043), (0.99163, 0.68408, 0.20706),
    (0.99314, 0.67408, 0.20348), (0.99438, 0.66386, 0.19971), (0.99535, 0.65341, 0.19577), (0.99607, 0.64277, 0.19165),
    (0.99654, 0.63193, 0.18738), (0.99675, 0.62093, 0.18297), (0.99672, 0.60977, 0.17842), (0.99644, 0.59846, 0.17376),
    (0.99593, 0.58703, 0.16899), (0.99517, 0.57549, 0.16412), (0.99419, 0.56386, 0.15918), (0.99297, 0.55214, 0.15417),
    (0.99153, 0.54036, 0.1491), (0.98987, 0.52854, 0.14398), (0.98799, 0.51667, 0.13883), (0.9859, 0.50479, 0.13367),
    (0.9836, 0.49291, 0.12849), (0.98108, 0.48104, 0.12332), (0.97837, 0.4692, 0.11817), (0.97545, 0.4574, 0.11305),
    (0.97234, 0.44565, 0.10797), (0.96904, 0.43399, 0.10294), (0.96555, 0.42241, 0.09798), (0.96187, 0.41093, 0.0931),
    (0.95801, 0.39958, 0.08831), (0.95398, 0.38836, 0.08362), (0.94977, 0.37729, 0.07905), (0.94538, 0.36638, 0.07461),
    (0.94084, 0.35566, 0.07031), (0.93612, 0.34513, 0.06616), (0.93125, 0.33482, 0.06218), (0.92623, 0.32473, 0.05837),
    (0.92105, 0.31489, 0.05475), (0.91572, 0.3053, 0.05134), (0.91024, 0.29599, 0.04814), (0.90463, 0.28696, 0.04516),
    (0.89888, 0.27824, 0.04243), (0.89298, 0.26981, 0.03993), (0.88691, 0.26152, 0.03753), (0.88066, 0.25334, 0.03521),
    (0.87422, 0.24526, 0.03297), (0.8676, 0.2373, 0.03082), (0.86079, 0.22945, 0.02875), (0.8538, 0.2217, 0.02677),
    (0.84662, 0.21407, 0.02487), (0.83926, 0.20654, 0.02305), (0.83172, 0.19912, 0.02131), (0.82399, 0.19182, 0.01966),
    (0.81608, 0.18462, 0.01809), (0.80799, 0.17753, 0.0166), (0.79971, 0.17055, 0.0152), (0.79125, 0.16368, 0.01387),
    (0.7826, 0.15693, 0.01264), (0.77377, 0.15028, 0.01148), (0.76476, 0.14374, 0.01041), (0.75556, 0.13731, 0.00942),
    (0.74617, 0.13098, 0.00851), (0.73661, 0.12477, 0.00769), (0.72686, 0.11867, 0.00695), (0.71692, 0.11268, 0.00629),
    (0.7068, 0.1068, 0.00571), (0.6965, 0.10102, 0.00522), (0.68602, 0.09536, 0.00481), (0.67535, 0.0898, 0.00449),
    (0.66449, 0.08436, 0.00424), (0.65345, 0.07902, 0.00408), (0.64223, 0.0738, 0.00401), (0.63082, 0.06868, 0.00401),
    (0.61923, 0.06367, 0.0041), (0.60746, 0.05878, 0.00427), (0.5955, 0.05399, 0.00453), (0.58336, 0.04931, 0.00486),
    (0.57103, 0.04474, 0.00529), (0.55852, 0.04028, 0.00579), (0.54583, 0.03593, 0.00638), (0.53295, 0.03169, 0.00705),
    (0.51989, 0.02756, 0.0078), (0.50664, 0.02354, 0.00863), (0.49321, 0.01963, 0.00955), (0.4796, 0.01583, 0.01055),
)


def colorwheel() -> np.ndarray:
    """float64 [55, 3]: make_colorwheel()'s integers."""
    return np.asarray(_WHEEL_DATA, dtype=np.float64)


def turbo_table() -> np.ndarray:
    """float64 [256, 3]: matplotlib.colormaps["turbo"](np.linspace(0, 1, 256))[:, :3]."""
    return np.asarray(_TURBO_DATA, dtype=np.float64)


def to_uint8(x: np.ndarray) -> np.ndarray:
    """The project's byte rule on a float32 video: min(255, max(0, x * 255 + 0.5)) in f32, truncated."""
    x = np.asarray(x, dtype=np.float32)
    return np.minimum(np.float32(255), np.maximum(np.float32(0), x * np.float32(255) + np.float32(0.5))).astype(np.uint8)


_TABLES: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}


def _tables(device):
    """(flipped turbo f32 [256, 3] as colormap_image holds it, colour wheel / 255.0 float64 [55, 3], hsv float64 [256, 3])."""
    if device not in _TABLES:
        turbo = torch.from_numpy(turbo_table()[::-1].copy()).to(torch.float32)  # torch.Tensor(...) then torch.flip (vis.py:264-268)
        _TABLES[device] = (turbo.contiguous().to(device), torch.from_numpy(colorwheel() / 255.0).contiguous().to(device),
                           torch.from_numpy(hsv_table()).contiguous().to(device))
    return _TABLES[device]


def panel_slots(tasks: List[str]) -> Dict[str, int]:
    """Panel slot of each visualised task in the reference's order (vis.py:56-94): rgb is slot 0, tasks without a panel (camray)
    take none."""
    slots: Dict[str, int] = {}
    for task in tasks:
        if task in PANEL_TASKS:
            if task in slots:
                raise ValueError(f"render_video_panels: task {task!r} is listed twice")
            slots[task] = len(slots) + 1
    return slots


def render_video_panels(batch: dict, out: dict, tasks: List[str], out_dtype=torch.float32) -> Dict[str, torch.Tensor]:
    """The panels of generate_video_visualizations as device tensors (csrc/vis2d.hip), batch element 0:

    video [T, H, P*W, 3] float32 (or uint8 by ``to_uint8``'s rule, written directly): the RGB panel, then one panel per entry of
        ``tasks`` among depth, flow_2d_backward, dyn_mask, track_2d, in that order;
    depth_range [2] float64 (vis.py:60-63; NaN and an all-zero panel when no depth is positive), flow_rad_max [1] float64
        (vis.py:413-418), as the reference holds them in Python floats; present whatever the tasks;
    with "track_2d", the display list: track_order_n [N] int32 (stable argsort of batch["track_2d_traj_bn2t"][0, :, 1, 0]),
        track_xy_tn2 [T, N, 2] int32 (estimates rounded half to even, sorted order), track_vis_tn [T, N] bool (sigmoid > 0.5 and
        finite coordinates), track_colors_n3 [N, 3] float32 (hsv of rank / (N - 1)).

    Nothing is read back and nothing synchronises: all sizes are static."""
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError("render_video_panels: out_dtype is torch.float32 or torch.uint8")
    rgb_in = batch["rgb_b3thw"]
    _, _, T, H, W = rgb_in.shape
    slots = panel_slots(tasks)
    keys = {"depth": "depth_est_b1thw", "flow_2d_backward": "flow_2d_backward_est_b2thw", "dyn_mask": "dyn_mask_est_b1thw",
            "track_2d": "track_2d_traj_est_bn2t"}
    dev = next((out[keys[t]].device for t in slots), torch.as_tensor(rgb_in).device)
    assert dev.type == "cuda", "render_video_panels runs on the GPU"
    lib, st = _lib.load(), _stream()
    turbo, wheel, hsv = _tables(dev)
    P = 1 + len(slots)
    u8 = out_dtype == torch.uint8
    rgb = _f32(rgb_in[0], dev)
    mean, std = _f32(batch["rgb_mean_b3111"][0], dev).reshape(3), _f32(batch["rgb_std_b3111"][0], dev).reshape(3)
    depth = _f32(out["depth_est_b1thw"][0, 0], dev) if "depth" in slots else None
    flow = _f32(out["flow_2d_backward_est_b2thw"][0], dev) if "flow_2d_backward" in slots else None
    mask = _f32(out["dyn_mask_est_b1thw"][0, 0], dev) if "dyn_mask" in slots else None
    for name, x, shape in (("rgb_b3thw", rgb, (3, T, H, W)), ("depth_est_b1thw", depth, (T, H, W)),
                           ("flow_2d_backward_est_b2thw", flow, (2, T, H, W)), ("dyn_mask_est_b1thw", mask, (T, H, W))):
        if x is not None and tuple(x.shape) != shape:
            raise ValueError(f"render_video_panels: {name}[0] has shape {tuple(x.shape)}, the video is {shape}")
    stats = torch.empty(3, dtype=torch.int32, device=dev)
    scalars = torch.empty(3, dtype=torch.float64, device=dev)
    video = torch.empty(T, H, P * W, 3, dtype=out_dtype, device=dev)
    track = "track_2d" in slots
    grey = torch.empty(T, H, W, dtype=torch.float32, device=dev) if (u8 and track) else None
    _lib.check(lib.l4p_vis_stats(st, _p(depth), _p(flow), T * H * W, _p(stats)), "l4p_vis_stats")
    _lib.check(lib.l4p_vis_panels(st, _p(rgb), _p(mean), _p(std), _p(depth), _p(flow), _p(mask), _p(stats), _p(turbo), _p(wheel),
                                  T, H, W, P, slots.get("depth", -1), slots.get("flow_2d_backward", -1), slots.get("dyn_mask", -1),
                                  slots.get("track_2d", -1), _p(video), int(u8), _p(grey), _p(scalars)), "l4p_vis_panels")
    res = {"video": video, "depth_range": scalars[:2], "flow_rad_max": scalars[2:]}
    if not track:
        return res
    key = _f32(batch["track_2d_traj_bn2t"][0], dev)  # the batch's trajectory, not the estimate (vis.py:454)
    traj = _f32(out["track_2d_traj_est_bn2t"][0], dev)
    logit = _f32(out["track_2d_vis_est_bn1t"][0, :, 0], dev)
    N = traj.shape[0]
    if tuple(traj.shape) != (N, 2, T) or tuple(logit.shape) != (N, T) or tuple(key.shape) != (N, 2, T):
        raise ValueError(f"render_video_panels: track tensors {tuple(key.shape)}, {tuple(traj.shape)}, {tuple(logit.shape)} do not "
                         f"describe N tracks over {T} frames")
    order = torch.empty(N, dtype=torch.int32, device=dev)
    xy = torch.empty(T, N, 2, dtype=torch.int32, device=dev)
    vis = torch.empty(T, N, dtype=torch.bool, device=dev)
    colors = torch.empty(N, 3, dtype=torch.float32, device=dev)
    if N > 0:
        _lib.check(lib.l4p_vis_track_prep(st, _p(key), _p(traj), _p(logit), _p(hsv), N, T, TRACK_VIS_THR, _p(order), _p(xy), _p(vis),
                                          _p(colors)), "l4p_vis_track_prep")
    row, p = P * W * 3, slots["track_2d"]
    if u8:
        src, s_px, s_row, s_frame = grey.data_ptr(), 1, W, H * W
        dst = video.data_ptr() + p * W * 3
    else:  # in place on the panel: the grey value sits in its channel 0
        src, s_px, s_row, s_frame = video.data_ptr() + p * W * 3 * 4, 3, row, H * row
        dst = src
    _lib.check(lib.l4p_vis_track_raster(st, _p(xy), _p(vis), _p(colors), N, T, H, W, TRACKS_LEAVE_TRACE, src, s_px, s_row, s_frame,
                                        dst, row, H * row, int(u8)), "l4p_vis_track_raster")
    res.update(track_order_n=order, track_xy_tn2=xy, track_vis_tn=vis, track_colors_n3=colors)
    return res


def write_png_frames(frames_u8: np.ndarray, directory: str) -> str:
    """uint8 frames [T, H, W, 3] as <directory>/<t:05d>.png (Pillow).  Returns the directory."""
    from PIL import Image

    os.makedirs(directory, exist_ok=True)
    for t, frame in enumerate(frames_u8):
        Image.fromarray(np.ascontiguousarray(frame), "RGB").save(os.path.join(directory, f"{t:05d}.png"))
    return directory


def read_png_frames(directory: str) -> np.ndarray:
    """Reader for what write_png_frames writes: uint8 [T, H, W, 3]."""
    from PIL import Image

    names = sorted(n for n in os.listdir(directory) if n.endswith(".png"))
    return np.stack([np.asarray(Image.open(os.path.join(directory, n)).convert("RGB")) for n in names])


def write_video(out_vid: np.ndarray, out_path: str, seq_name: str) -> str:
    """<out_path>/<seq_name>.mp4 at 15 fps through mediapy where it is importable (vis.py:99-100; mediapy is not installed where
    this was written, so that branch has never run here), else the uint8 frames as PNG files under <out_path>/<seq_name>/.  A uint8
    video (utils/view4d.py) is written as it is."""
    os.makedirs(out_path, exist_ok=True)
    try:
        import mediapy as media
    except ImportError:
        frames = out_vid if np.asarray(out_vid).dtype == np.uint8 else to_uint8(out_vid)
        return write_png_frames(frames, os.path.join(out_path, seq_name))
    name = os.path.join(out_path, f"{seq_name}.mp4")
    media.write_video(name, out_vid, fps=FPS)
    return name


def generate_video_visualizations(batch, out, tasks, out_path=None) -> Tuple[np.ndarray, Optional[str]]:
    """vis.py:34-104 on the GPU: returns (out_vid float32 [T, H, P*W, 3] on the host, the name of what was written or None).  One
    device-to-host copy.  With out_path: <out_path>/<seq_name>.mp4 at 15 fps if mediapy is importable (a branch that cannot be
    exercised where this was written), otherwise PNG frames <out_path>/<seq_name>/<t:05d>.png and that directory's name."""
    seq_name = batch["seq_name"][0]
    out_vid = render_video_panels(batch, out, tasks)["video"].cpu().numpy()
    name = write_video(out_vid, out_path, seq_name) if out_path is not None else None
    return out_vid, name
