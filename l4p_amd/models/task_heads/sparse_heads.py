"""SAM-style 2D/3D point tracker on the MI355X engine — host mirror of
l4p/models/task_heads/sparse_heads.py (+ sam/prompt_encoder.py, sam/transformer.py, sam/mask_decoder.py).

Same class name, constructor arguments, ``forward_windowed`` / ``forward`` signatures and output keys as
the reference.  All arithmetic — projections (MFMA GEMM), the three small-token attention shapes,
LayerNorms, up-scaling ConvTransposes, hyper-network product, the fused up-sample + soft-argmax read-out
and the integer/boolean sliding-window bookkeeping — runs in libl4p_hip.so; the Python below only
sequences kernels over device buffers (no host synchronisation inside a window).
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, List, Literal, Optional, Tuple

import torch

from ... import _lib
from ...ops import _p, _stream


class VideoMAETrack2DSamHead(torch.nn.Module):
    def __init__(
        self,
        task_name: str = "track_2d",
        prompt_embed_dim: int = 1408,
        image_size: Tuple[int, int, int] = (16, 224, 224),
        patch_size: Tuple[int, int, int] = (2, 14, 14),
        estimate_vis: bool = False,
        estimate_depth: bool = False,
        sam_head_depth: int = 2,
        decoding_out_dim_factor: int = 8,
        num_prompt_points: int = 2,
        num_point_embeddings: int = 2,
        modify_pointlabels_for_windowing: bool = False,
        prompt_using_features: bool = False,
        attend_to_past: bool = False,
        depth_fn: str = "linear",
        vis_fn: str = "linear",
        estimation_directions: List[Literal[1, -1]] = [1, -1],
        max_queries: int = 192,
    ):
        super().__init__()
        # the engine implements the configuration shipped in configs/model.yaml:53-66
        if not (estimate_vis and estimate_depth and prompt_using_features and attend_to_past and
                modify_pointlabels_for_windowing and num_point_embeddings == 2 and num_prompt_points == 2 and
                depth_fn == "exp" and vis_fn == "linear"):
            raise NotImplementedError("tracker options other than those of configs/model.yaml are not built into the engine")
        self.task_name = task_name
        self.prompt_embed_dim = prompt_embed_dim
        self.image_size = tuple(image_size)
        self.patch_size = tuple(patch_size)
        self.sam_head_depth = sam_head_depth
        self.decoding_out_dim_factor = decoding_out_dim_factor
        self.estimation_directions = list(estimation_directions)
        self.max_queries = max_queries
        self.image_embedding_size = tuple(int(image_size[i] / patch_size[i]) for i in range(3))
        self.video_tokens_size = self.image_embedding_size[0] * self.image_embedding_size[1] * self.image_embedding_size[2]
        self.task_suffix = "_track_2d"
        self._rt = None
        self._engine_task = ""
        self.trace: Optional[list] = None  # set to [] to record per-window labels / queries (tests)
        self._direction: Optional[int] = None  # the pass of a two-direction call that is running (select_direction)

    # ------------------------------------------------------------------------------------------------
    def _single_window_history_rows(self, N: int, P: int) -> int:
        return P  # (a single window only reads the shared first P rows; tests override this to exercise the general path)

    def _w(self, k: str) -> torch.Tensor:
        return self._rt.weights["trk." + k]

    # ------------------------------------------------------------------------------------------------
    def _window(self, enc_last: torch.Tensor, hist: torch.Tensor, q_off: torch.Tensor, labels: torch.Tensor,
                pfeat: torch.Tensor, plabel: torch.Tensor, need_history: bool, hist_uniform: int = 0):
        """forward / forward_single_batch (sparse_heads.py:497-667) for N queries of one clip.
        enc_last: float [P,C]; hist: float [N,P,C]; returns window traj [N,2,T], vis [N,T], depth [N,T],
        new prompt features [N,C]; updates ``hist`` in place when ``need_history``.
        ``hist_uniform``: every track has the same history rows (first window: the learned mask token), so until the
        first image->token update the keys are ONE [P,C] set: the first layer's t2i.k / t2i.v / i2t.q projections and
        the key initialisation run once instead of N times (identical rows in, identical rows out)."""
        rt = self._rt
        cfg = rt.cfg
        eng = getattr(rt, "engine", None)
        if eng is None:
            raise RuntimeError("tracker head has no engine: the window runs as one native call (l4p_track_window_forward)")
        # the whole window as ONE native call (csrc/api_trackwin.hip: the statement of the window's graph and of its switches)
        tc = _lib.TrackCfg(dim=cfg.dim, tokens=cfg.tokens, nt=cfg.grid[0], nh=cfg.grid[1], nw=cfg.grid[2],
                           sam_depth=cfg.sam_depth, sam_heads=cfg.sam_heads, sam_mlp=cfg.sam_mlp,
                           out_dim_factor=self.decoding_out_dim_factor, T=self.image_size[0], H=self.image_size[1],
                           W=self.image_size[2])
        return eng.track_window(tc, enc_last, hist, q_off, labels, pfeat, plabel, need_history, hist_uniform,
                                slot=getattr(self, "_ws_slot", 0))

    # ------------------------------------------------------------------------------------------------
    def forward_windowed(self, enc_features_bpc_2dlist, track_2d_pointquerries_bn3: torch.Tensor,
                         track_2d_pointlabels_bn: torch.Tensor, time_strides: Optional[torch.Tensor] = None,
                         **kwargs) -> Dict[str, torch.Tensor]:
        """Chunks of ``max_queries`` (sparse_heads.py:162-211)."""
        N = track_2d_pointquerries_bn3.shape[1]
        if N < self.max_queries:
            return self.forward_windowed_core(enc_features_bpc_2dlist, track_2d_pointquerries_bn3, track_2d_pointlabels_bn,
                                              time_strides, **kwargs)
        outs = []
        for i in range(int(math.ceil(N / self.max_queries))):
            sl = slice(i * self.max_queries, (i + 1) * self.max_queries)
            outs.append(self.forward_windowed_core(enc_features_bpc_2dlist, track_2d_pointquerries_bn3[:, sl],
                                                   track_2d_pointlabels_bn[:, sl], time_strides, **kwargs))
        # The concatenation below reads every chunk's buffers on the launching stream: with a deferred join the clip streams
        # may still be writing them (and the chunk buffers would go back to the allocator while in use).  Join here; the
        # chunks of one clip already ran back to back on that clip's stream.
        self.join_streams()
        return {k: torch.cat([o[k] for o in outs], dim=1) for k in outs[0]}

    def forward_windowed_core(self, enc_features_bpc_2dlist, track_2d_pointquerries_bn3: torch.Tensor,
                              track_2d_pointlabels_bn: torch.Tensor, time_strides: Optional[torch.Tensor] = None,
                              **kwargs) -> Dict[str, torch.Tensor]:
        """Causal sliding-window tracking (sparse_heads.py:213-495): ONE pass in the positive time direction.  With -1 among
        estimation_directions the second pass is this same recursion on the time-flipped clip, and L4P_VideoMAE.forward is what
        flips, runs and merges (the reference's recipe, sparse_heads.py:242-245); it says which pass this is through
        ``select_direction``."""
        if self._rt is None:
            raise RuntimeError("tracker head has no weights: call load_state_dict on the model first")
        direction = self.pass_direction()
        if time_strides is None:  # if windowing is not needed just do a forward pass (sparse_heads.py:223-227)
            return self.forward(enc_features_bpc_2dlist[0], track_2d_pointquerries_bn3, track_2d_pointlabels_bn)
        lib = _lib.load()
        cfg = self._rt.cfg
        dev = enc_features_bpc_2dlist[0].f32(-1).device
        ws = self.image_size[0]
        B = track_2d_pointquerries_bn3.shape[0]
        N = track_2d_pointquerries_bn3.shape[1]
        T = int(time_strides[-1]) + ws
        if N == 0:  # no queries: the reference's buffers with an empty query axis (sparse_heads.py:233-239), no kernel to launch
            z = dict(dtype=torch.float32, device=dev)
            return {f"{self.task_name}_traj_est_bn2t": torch.zeros(B, 0, 2, T, **z),
                    f"{self.task_name}_vis_est_bn1t": torch.full((B, 0, 1, T), -10.0, **z),
                    f"{self.task_name}_depth_est_bn1t": torch.zeros(B, 0, 1, T, **z)}
        P, Cc = cfg.tokens, cfg.dim
        f32 = dict(dtype=torch.float32, device=dev)
        def output_buffers():
            return (torch.zeros(B, N, 2, T, **f32), torch.full((B, N, 1, T), -10.0, **f32), torch.zeros(B, N, 1, T, **f32))

        # (start_event: the clip streams wait for that event only, not for what the launching stream has queued since - the fills
        #  of the output buffers must then run on a clip stream too, or they would land behind that queue and wipe the results)
        early = (getattr(self, "start_event", None) is not None and bool(getattr(self, "own_stream", False)) and dev.type == "cuda"
                 and os.environ.get("L4P_TRACK_STREAMS", "1") != "0")
        traj_all = vis_all = dep_all = None
        if not early:
            traj_all, vis_all, dep_all = output_buffers()
        nwin = len(time_strides)
        # Clips are independent (the reference asserts B == 1, sparse_heads.py:241).  Each clip's tracker runs on its own
        # HIP stream: its many token-side launches are tiny (M = 6N rows -> a few dozen workgroups) and leave most CUs
        # idle, so the clips fill each other's gaps.
        def run_clip(b: int) -> None:
            orig_q = track_2d_pointquerries_bn3[b].to(**f32).contiguous()
            cur_q = orig_q.clone()
            pfeat = torch.zeros(N, Cc, **f32)
            plabel = torch.zeros(N, **f32)
            # history tokens: the learned mask token everywhere before the first window; a single window only ever reads
            # the first P rows (shared keys), so the per-track copy is not materialised for it
            hrows = N * P if nwin > 1 else self._single_window_history_rows(N, P)
            hist = torch.empty(hrows, Cc, **f32)
            _lib.check(lib.l4p_fill_rows(_stream(), _p(hist), _p(self._w("history_mask_token")), hrows, Cc, hrows, 0, 0),
                       "l4p_fill_rows")
            q_off = torch.empty(N, 3, **f32)
            labels = torch.empty(N, **f32)
            valid_t = torch.empty(N, ws, dtype=torch.uint8, device=dev)
            valid_n = torch.empty(N, dtype=torch.uint8, device=dev)
            best = torch.zeros(N, dtype=torch.int32, device=dev)
            traj_b, vis_b, dep_b = traj_all[b], vis_all[b, :, 0], dep_all[b, :, 0]  # (late binding: set before any clip runs)
            for wi in range(nwin):
                start = int(time_strides[wi])
                last = wi == nwin - 1
                nxt = int(time_strides[wi + 1]) if not last else start
                _lib.check(lib.l4p_track_prepare(_stream(), _p(cur_q), _p(orig_q), start, ws, _p(q_off), _p(labels),
                                                 _p(valid_t), _p(valid_n), N), "l4p_track_prepare")
                if self.trace is not None:
                    # (recorded on whatever stream the clip runs on: the clones are ordered behind track_prepare there, so
                    # tracing does not change the schedule — the benchmarked stream configuration can be traced as it runs)
                    self.trace.append({"clip": b, "window": wi, "labels": labels.clone(), "queries": q_off.clone(),
                                       "prompt_labels": plabel.clone(), "valid_t": valid_t.clone()})
                    if direction is not None:  # (a pass of a model that tracks in both directions: which one)
                        self.trace[-1]["direction"] = direction
                enc_last = enc_features_bpc_2dlist[wi].f32(-1)[b].contiguous()
                # first window: the history of every track is the learned mask token (filled above) -> shared keys
                # later windows: the second temporal half of every track's history is the mask token again (written by the
                # previous window's memory update) -> what layer 0 derives from those rows is computed once (L4P_TRACK_HALF_SHARE=0:
                # every track on its own, the A/B and equality check)
                hu = 1 if wi == 0 else (2 if os.environ.get("L4P_TRACK_HALF_SHARE", "1") != "0" else 4)  # (4: a later window, every track on its own rows)
                # (need_history = 2: hist was filled with the mask token above and only this loop writes it - the memory update
                #  of a window rewrites rows [0, P/2) of each track, nothing touches rows [P/2, P) - so the re-fill is skipped)
                w_traj, w_vis, w_dep, new_pfeat = self._window(enc_last, hist, q_off, labels, pfeat, plabel, 0 if last else 2,
                                                               hist_uniform=hu)
                _lib.check(lib.l4p_track_commit(_stream(), _p(w_traj), _p(w_vis), _p(w_dep), _p(valid_t), _p(valid_n),
                                                traj_b.data_ptr(), vis_b.data_ptr(), dep_b.data_ptr(), T, start, ws, nxt,
                                                1 if last else 0, _p(cur_q), _p(plabel), _p(new_pfeat), _p(pfeat), _p(best),
                                                N, Cc), "l4p_track_commit")
                if self.trace is not None and not last:
                    self.trace[-1]["best_vis_id"] = best.clone()

        # (own_stream: a single clip goes to a stream of its own as well - parallel.forward_windows_sharded starts the recursion
        #  of a long video before the dense decoders and joins it before the seam alignment)
        use_streams = ((B > 1 or bool(getattr(self, "own_stream", False))) and dev.type == "cuda"
                       and os.environ.get("L4P_TRACK_STREAMS", "1") != "0")
        if use_streams:
            main = torch.cuda.current_stream()
            pool = getattr(self, "clip_stream_override", None)  # (the caller's streams: parallel.forward_windows_sharded, CU-masked)
            if pool is None or len(pool) < B:
                pool = getattr(self, "_clip_streams", None)
            if pool is None or len(pool) < B:
                # (L4P_TRACK_PRIO=1: high-priority clip streams.  Measured, round 4, same call: c3 832 -> 654 frames/s - at 64 queries
                #  the tracker's kernels are chip-sized themselves and pre-empt the decoders' rounds -, configs[4] 414 -> 415: off)
                prio = -1 if os.environ.get("L4P_TRACK_PRIO", "0") == "1" else 0
                pool = [torch.cuda.Stream(device=dev, priority=prio) for _ in range(B)]
                self._clip_streams = pool
            start = getattr(self, "start_event", None) if early else None  # what the clip streams wait for: an event of the
            if start is not None:                       # launching stream (parallel.forward_windows_sharded), else everything
                pool[0].wait_event(start)               # queued on it so far
                with torch.cuda.stream(pool[0]):
                    traj_all, vis_all, dep_all = output_buffers()
                # allocated on a clip stream, handed to the launching stream's consumers after the join: the allocator must not
                # hand the blocks out again (to pool[0]) while work queued on the launching stream still reads them
                for t in (traj_all, vis_all, dep_all):
                    t.record_stream(main)
            for b in range(B):
                if start is None:
                    pool[b].wait_stream(main)
                elif b > 0:
                    pool[b].wait_stream(pool[0])
                with torch.cuda.stream(pool[b]):
                    self._ws_slot = b + 1  # concurrent clips: one native workspace each
                    run_clip(b)
            self._ws_slot = 0
            if getattr(self, "defer_join", False):
                # the caller (L4P_VideoMAE.stitch_windows) runs the dense heads on the main stream meanwhile and joins the
                # clip streams before it returns: the tracker's ~130 tiny dependent launches per clip fill the gaps of the
                # decoders' large kernels instead of serialising in front of them
                self._pending = (main, pool[:B])
            else:
                for b in range(B):
                    main.wait_stream(pool[b])
        else:
            for b in range(B):
                run_clip(b)
        return {f"{self.task_name}_traj_est_bn2t": traj_all, f"{self.task_name}_vis_est_bn1t": vis_all,
                f"{self.task_name}_depth_est_bn1t": dep_all}

    def pass_direction(self) -> Optional[int]:
        """None with estimation_directions [1] (the one pass there is); else the direction of the pass L4P_VideoMAE.forward has
        selected.  With -1 configured and no pass selected the head was called on its own: one causal pass would silently return one
        direction where two were asked for, so it raises."""
        dirs = sorted(self.estimation_directions)
        if dirs == [1]:
            return None
        if dirs not in ([-1], [-1, 1]):
            raise ValueError(f"estimation_directions {self.estimation_directions}: expected [1], [-1], [1, -1] or [-1, 1]")
        if self._direction is None:
            raise RuntimeError(
                f"estimation_directions {self.estimation_directions}: the tracker head runs one causal pass; the reversed pass on the "
                "time-flipped clip and the merge of the two are made by L4P_VideoMAE.forward - call that, not the head")
        return self._direction

    @contextlib.contextmanager
    def select_direction(self, direction: int):
        """L4P_VideoMAE.forward: the windowed passes run inside are the ``direction`` pass of a two-direction call."""
        saved, self._direction = self._direction, int(direction)
        try:
            yield
        finally:
            self._direction = saved

    def join_streams(self) -> None:
        """Make the stream that launched the tracker wait for the clip streams (no-op when nothing is pending)."""
        pend = getattr(self, "_pending", None)
        if pend is not None:
            main, pool = pend
            for st in pool:
                main.wait_stream(st)
            self._pending = None

    def forward(self, enc_features_bpc_list, track_2d_pointquerries_bn3: torch.Tensor, track_2d_pointlabels_bn: torch.Tensor,
                track_2d_promptfeatures_bnc: Optional[torch.Tensor] = None,
                track_2d_promptfeaturelabels_bn: Optional[torch.Tensor] = None, **kwargs) -> Dict[str, torch.Tensor]:
        """Single-window forward (sparse_heads.py:497-600), reached from L4P_VideoMAE.forward_single_window
        (always_use_windowed_version=False and T == 16) and from forward_windowed_core(time_strides=None).  Unlike a window of
        the sliding tracker it attends to the raw enc_features[-1] (NO history / mask-token term), takes the caller's point
        labels as they are, starts from zero prompt features unless they are passed in, and returns the window's estimates
        for every frame (no validity masking, no -10 visibility fill).
        Returned: traj [B,N,2,T], vis [B,N,1,T], depth [B,N,1,T], <task>_prompt_features_bnc [B,N,C] and, as the reference
        (sparse_heads.py:560-569), <task>_enc_features_with_track_history_bnpc [B,N,P,C] float - the projection of every
        processed video token (11.5 MB per query at the full geometry: ``self.return_track_history = False`` skips it)."""
        if self._rt is None:
            raise RuntimeError("tracker head has no weights: call load_state_dict on the model first")
        lib = _lib.load()
        cfg = self._rt.cfg
        enc = enc_features_bpc_list.f32(-1)
        dev = enc.device
        B, N = track_2d_pointquerries_bn3.shape[:2]
        T = self.image_size[0]
        P, Cc = cfg.tokens, cfg.dim
        f32 = dict(dtype=torch.float32, device=dev)
        traj_all = torch.empty(B, N, 2, T, **f32)
        vis_all = torch.empty(B, N, 1, T, **f32)
        dep_all = torch.empty(B, N, 1, T, **f32)
        pf_all = torch.empty(B, N, Cc, **f32)
        zero_hist = torch.zeros(P, Cc, **f32)  # keys = enc_features[-1] + 0: one key set shared by all tracks
        # the reference returns the [B,N,P,C] float history from this entry unconditionally (sparse_heads.py:560-569), so the
        # default keeps the key; it costs 11.5 MB and one P x C x C projection per query (0.74 GB per clip at 64 queries): a
        # caller that only wants the trajectories sets ``head.return_track_history = False``.  The sliding-window path
        # (forward_windowed_core with time strides - what bench.py and the demo run) never materialises it.
        want_hist = bool(getattr(self, "return_track_history", True))
        hist_all = torch.empty(B, N, P, Cc, **f32) if want_hist else None
        for b in range(B):
            q = track_2d_pointquerries_bn3[b].to(**f32).contiguous()
            labels = track_2d_pointlabels_bn[b].to(**f32).contiguous()
            pfeat = (torch.zeros(N, Cc, **f32) if track_2d_promptfeatures_bnc is None
                     else track_2d_promptfeatures_bnc[b].to(**f32).contiguous())
            plabel = (torch.zeros(N, **f32) if track_2d_promptfeaturelabels_bn is None
                      else track_2d_promptfeaturelabels_bn[b].to(**f32).contiguous())
            if want_hist:
                # hist [N*P, C]: its first P rows are the (zero) history the shared keys are built from, the call then
                # overwrites all of it with the projection of the processed tokens (need_history = 3)
                hist = hist_all[b].view(N * P, Cc)
                hist[:P].zero_()
            else:
                hist = zero_hist
            w_traj, w_vis, w_dep, new_pfeat = self._window(enc[b].contiguous(), hist, q, labels, pfeat, plabel,
                                                           3 if want_hist else 0, hist_uniform=True)
            traj_all[b], vis_all[b, :, 0], dep_all[b, :, 0], pf_all[b] = w_traj, w_vis, w_dep, new_pfeat
        out = {f"{self.task_name}_traj_est_bn2t": traj_all, f"{self.task_name}_vis_est_bn1t": vis_all,
               f"{self.task_name}_depth_est_bn1t": dep_all, f"{self.task_name}_prompt_features_bnc": pf_all}
        if want_hist:
            out[f"{self.task_name}_enc_features_with_track_history_bnpc"] = hist_all
        return out
