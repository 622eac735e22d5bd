"""Host-side driver of the HIP scoring path: owns the packed weights handle and the small per-config
device tables, and turns torch CUDA tensors into raw pointers for the C ABI (include/mocodad_hip.h).
PyTorch is used for device memory and streams only; every FLOP of the path runs in libmocodad_hip.so."""
import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .utils.diffusion_utils import latent_step_table, step_table


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def _i32c(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.int32).contiguous()


def _quantile_of(strategy: str) -> float:
    """'quantile:q' -> q, rejected outside [0, 1] like torch.quantile does (mocodad.py:513-516)."""
    try:
        q = float(strategy.split(":")[-1])
    except ValueError:
        raise ValueError(f"bad quantile in aggregation strategy {strategy!r}") from None
    if not 0.0 <= q <= 1.0:      # (NaN fails too)
        raise ValueError(f"quantile() q must be in the range [0, 1], got {q} ({strategy!r})")
    return q


LOSS_AGGREGATIONS = ("best", "worst", "mean", "median", "quantile")


def _aggregation_of(strategy: str, allowed, error: str) -> Tuple[str, float]:
    """'best' | ... | 'quantile:q' -> (name in _lib.AGGR, q); ValueError(error) for a name outside `allowed`."""
    name, q = strategy, 0.0
    if "quantile" in strategy:
        q, name = _quantile_of(strategy), "quantile"
    if name not in allowed:
        raise ValueError(error)
    return name, q


def _seed64(seed: int):
    return C.c_uint64(seed & (2**64 - 1))


def _need_gpu() -> None:
    if not torch.cuda.is_available():
        raise RuntimeError("mocodad_amd needs an MI355X (gfx950) GPU: the scoring path has no CPU fallback")


def _out_vector(out: Optional[torch.Tensor], B: int, device) -> torch.Tensor:
    """The (B,) fp32 result vector of a call: the caller's preallocated `out`, checked, or a new one."""
    if out is None:
        return torch.empty(B, device=device, dtype=torch.float32)
    if out.shape != (B,) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise ValueError("out must be a contiguous float32 (B,) tensor on the scorer's device")
    return out


def _window_view(wb=None, cond_mask: Optional[torch.Tensor] = None) -> "_lib.WindowView":
    """mcd_window_view_t of a WindowBatch (None: dense windows) and / or per-window condition-frame bitmasks."""
    mask = cond_mask.data_ptr() if cond_mask is not None else None
    if wb is None:
        return _lib.WindowView(base=None, stride_c=0, stride_t=0, trans=None, affine=None, cond_mask=mask)
    return _lib.WindowView(base=wb.base.data_ptr(), stride_c=wb.stride_c, stride_t=wb.stride_t,
                           trans=wb.trans.data_ptr() if wb.trans is not None else None,
                           affine=wb.affine.data_ptr() if wb.affine is not None else None, cond_mask=mask)


def _pack_tensors(state_dict):
    """state_dict -> (ctypes array of mcd_tensor_t, count, host copies to keep alive during the call)."""
    keep = []
    arr = (_lib.Tensor * len(state_dict))()
    n = 0
    for k, v in state_dict.items():
        if not torch.is_tensor(v) or not v.dtype.is_floating_point:
            continue
        h = v.detach().to("cpu", torch.float32).contiguous()
        keep.append(h)
        arr[n].name = k.encode()
        arr[n].data = h.data_ptr()
        arr[n].numel = h.numel()
        n += 1
    return arr, n, keep


class _Scorer:
    """What HipScorer and LatentScorer share: the model's frame lists and sizes, the per-call config, the step-table cache, one
    workspace per stream, the handle's options and its release.  A subclass names its library entries and its step table."""

    _OPTIONS: Dict[str, int] = {}       # option name -> id, and the entries that set one / free the handle
    _SET_OPTION = _FREE = ""
    _step_table = None

    def _init_model(self, seg_len, cond_idx, corrupt_idx, num_coords, n_joints, emb_dim) -> None:
        self.L = _lib.lib()
        self._h = None
        self.seg_len = int(seg_len)
        self.cond_idx = [int(i) for i in cond_idx]
        self.corrupt_idx = [int(i) for i in corrupt_idx]
        self.num_coords, self.n_joints, self.emb_dim = num_coords, n_joints, emb_dim
        self._tables: Dict[int, torch.Tensor] = {}
        self._ws: Dict[int, torch.Tensor] = {}   # workspace, one per stream (launches on different streams may overlap, each
        #                                          needs its own)
        self._map_bufs: Dict[tuple, torch.Tensor] = {}   # want_maps: poses / per-sample losses nobody asked for, per stream

    def _model_cfg(self, strategy: str, t_unet: int, t_cond: int, cond_channels, cond_unet: bool) -> "_lib.ModelCfg":
        cfg = _lib.ModelCfg()
        cfg.num_coords, cfg.n_joints, cfg.t_unet, cfg.t_cond = self.num_coords, self.n_joints, t_unet, t_cond
        cfg.emb_dim, cfg.strategy = self.emb_dim, _lib.STRATEGY[strategy]
        if strategy == "inject" and cond_unet:      # 'E_unet' condition encoder (the U-Net's down path)
            cfg.cond_layers = _lib.COND_UNET
        else:
            cfg.cond_layers = len(cond_channels) if strategy == "inject" else 0
            for i, c in enumerate(cond_channels):
                cfg.cond_channels[i] = int(c)
        return cfg

    def _set_options(self, options: Optional[Dict[str, int]]) -> None:
        for name, value in (options or {}).items():
            self.set_option(name, value)

    def set_option(self, name: str, value: int) -> None:
        """Per-handle switch of the library (include/mocodad_hip.h): MCD_OPT_* 'variant', 'cond_generic', 'generic_unet', 'split',
        'phase' on a HipScorer; MCD_LATENT_OPT_* 'split_encode' on a LatentScorer (1 makes the shipped configuration take the
        three-launch form, condition encoder as its own launch, as well); 'decode_spw' / 'decode_chunk' on a LatentReconstructor
        (test aids of decode_samples: samples per workgroup, windows per chunk; 0 = the library's rules; no result depends on them)."""
        if name not in self._OPTIONS:
            raise ValueError(f"unknown option {name!r} (known: {sorted(self._OPTIONS)})")
        _lib.check(getattr(self.L, self._SET_OPTION)(self._h, self._OPTIONS[name], int(value)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                getattr(self.L, self._FREE)(h)
            except Exception:
                pass
            self._h = None

    def table(self, noise_steps: int) -> torch.Tensor:
        t = self._tables.get(noise_steps)
        if t is None:
            t = self._step_table(noise_steps, self.emb_dim).to(self.device)
            self._tables[noise_steps] = t
        return t

    def _score_cfg(self, B: int, S: int, ns: int, loss_fn: str = "smooth_l1") -> "_lib.ScoreCfg":
        c = _lib.ScoreCfg()
        c.n_windows, c.n_samples, c.noise_steps, c.seg_len = B, S, ns, self.seg_len
        c.n_cond, c.n_corrupt = len(self.cond_idx), len(self.corrupt_idx)
        for i, v in enumerate(self.cond_idx):
            c.cond_idx[i] = v
        for i, v in enumerate(self.corrupt_idx):
            c.corrupt_idx[i] = v
        c.loss_fn = _lib.LOSS[loss_fn]
        return c

    def _workspace(self, need: int) -> torch.Tensor:
        """The current stream's workspace, at least `need` bytes.  Call inside `torch.cuda.device(self.device)`."""
        sid = torch.cuda.current_stream().cuda_stream
        ws = self._ws.get(sid)
        if ws is None or ws.numel() < need:
            ws = self._ws[sid] = torch.empty(max(need, 256), device=self.device, dtype=torch.uint8)
        return ws

    def _check_shape(self, what: str, t: torch.Tensor, tail: Tuple[int, ...]) -> None:
        if t.dim() != len(tail) + 1 or tuple(t.shape[1:]) != tuple(tail):
            raise ValueError(f"{what} must have shape (B, {', '.join(map(str, tail))}), got {tuple(t.shape)}")

    def _windows(self, data, cond_mask: Optional[torch.Tensor] = None):
        """(B,C,T,V) tensor or WindowBatch, (B,) int32 device bitmasks | None -> (data tensor, WindowView | None, B, keep-alive)"""
        if hasattr(data, "as_view"):
            wb = data.to(self.device)
            if wb.seg_len != self.seg_len:
                raise ValueError(f"window view has seg_len {wb.seg_len}, model expects {self.seg_len}")
            out = wb.buffer, _window_view(wb, cond_mask), int(wb.base.shape[0]), wb
        else:
            self._check_shape("data", data, (self.num_coords, self.seg_len, self.n_joints))
            data = _f32c(data, self.device)
            # (dense windows need a view only for their per-window condition sets)
            out = data, _window_view(None, cond_mask) if cond_mask is not None else None, int(data.shape[0]), None
        if cond_mask is not None and cond_mask.numel() != out[2]:
            raise ValueError(f"cond_mask must have {out[2]} entries")
        return out


    # ------------------------------------------------------------------ handle-free entries on poses: any scorer whose calls
    # yield (loss_all (B,S), poses_all (B,S,C,Tx,V)) -- HipScorer.score, LatentReconstructor.decode_samples -- has them
    def _scratch(self, kind: str, numel: int) -> torch.Tensor:
        """`numel` floats of the current stream's scratch buffer `kind` (the poses / per-sample losses a maps launch reads when the
        caller did not ask for them): grown on demand, reused by the next call.  Call inside `torch.cuda.device(self.device)`."""
        key = (kind, torch.cuda.current_stream().cuda_stream)
        buf = self._map_bufs.get(key)
        if buf is None or buf.numel() < numel:
            buf = self._map_bufs[key] = torch.empty(max(numel, 1), device=self.device, dtype=torch.float32)
        return buf[:numel]

    def error_maps(self, data, loss_all: Optional[torch.Tensor], poses_all: torch.Tensor, strategy: str, *, loss_fn: str = "smooth_l1",
                   cond_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mcd_error_maps: which joints and forecast frames a window's score comes from.  data: the windows the poses were
        scored on ((B,C,T,V) tensor or WindowBatch: the ground truth is read through the view, transform applied); loss_all (B,S)
        (None for 'all', 'mean', 'mean_pose', 'median_pose', which do not read it); poses_all (B,S,C,Tx,V); strategy: 'all' |
        'best' | 'worst' | 'mean' | 'median' | 'quantile:q' | 'mean_pose' | 'median_pose' -> M (B,Tx,V), for 'all' E (B,S,Tx,V).
        cond_mask ('random_imp'): the batch's (B,) condition-frame bitmasks.  Asynchronous on the current stream."""
        name, q = _aggregation_of(strategy, list(_lib.AGGR), f"Unknown aggregation strategy {strategy}")
        if cond_mask is not None:
            cond_mask = cond_mask.to(self.device, torch.int32).contiguous()
        data, view, B, keep = self._windows(data, cond_mask)
        poses_all = _f32c(poses_all, self.device)
        Tx = len(self.corrupt_idx)
        if poses_all.dim() != 5 or poses_all.shape[0] != B or tuple(poses_all.shape[2:]) != (self.num_coords, Tx, self.n_joints):
            raise ValueError(f"poses_all must have shape ({B}, S, {self.num_coords}, {Tx}, {self.n_joints}), got {tuple(poses_all.shape)}")
        S = int(poses_all.shape[1])
        if loss_all is not None:
            loss_all = _f32c(loss_all, self.device)
            if tuple(loss_all.shape) != (B, S):
                raise ValueError(f"loss_all must have shape ({B}, {S}), got {tuple(loss_all.shape)}")
        elif name not in ("all", "mean", "mean_pose", "median_pose"):
            raise ValueError(f"the {name!r} maps select samples by their losses: loss_all is required")
        with torch.cuda.device(self.device):
            maps = self._maps_launch(data, view, B, S, name, q, loss_all, poses_all, loss_fn)
        del keep
        return maps

    def _maps_launch(self, data, view, B, S, name, q, loss_all, poses_all, loss_fn) -> torch.Tensor:
        Tx = len(self.corrupt_idx)
        shape = (B, S, Tx, self.n_joints) if name == "all" else (B, Tx, self.n_joints)
        maps = torch.empty(shape, device=self.device, dtype=torch.float32)
        cfg = self._score_cfg(B, S, 2, loss_fn)
        _lib.check(self.L.mcd_error_maps(C.byref(cfg), self.num_coords, self.n_joints, _lib.AGGR[name], C.c_float(q), _ptr(loss_all),
                                         _ptr(poses_all), _ptr(data), C.byref(view) if view is not None else None, _ptr(maps),
                                         _stream()))
        return maps

    def joint_scatter_max(self, maps: torch.Tensor, frames: torch.Tensor, row: torch.Tensor, n_rows: int, n_frames: int) -> torch.Tensor:
        """mcd_joint_scatter_max: maps (N,Tx,V), frames (N,Tx) 1-based frame id of each map row, row (N,) output row
        -> (n_rows, n_frames, V): per joint the maximum over the windows forecasting the frame; 0 where none does."""
        maps, frames, row = _f32c(maps, self.device), _i32c(frames, self.device), _i32c(row, self.device)
        n = int(row.numel())
        if maps.dim() != 3 or maps.shape[0] != n or maps.shape[2] != 17 or tuple(frames.shape) != (n, maps.shape[1]):
            raise ValueError(f"need maps (N, Tx, 17), frames (N, Tx) and row (N,), got {tuple(maps.shape)}, {tuple(frames.shape)}, {tuple(row.shape)}")
        out = torch.empty(int(n_rows), int(n_frames), 17, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_joint_scatter_max(_ptr(maps), _ptr(frames), _ptr(row), n, int(maps.shape[1]), int(n_rows), int(n_frames),
                                                    _ptr(out), _stream()))
        return out

    def aggregate(self, data: torch.Tensor, loss_all: torch.Tensor, poses_all: Optional[torch.Tensor], strategy: str,
                  *, noise_steps: int, loss_fn: str = "smooth_l1", want_pose: bool = True,
                  out: Optional[torch.Tensor] = None, cond_mask: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """_aggregation_strategy of the reference on device -> (selected pose | None, loss (B,)).
        out: optional preallocated contiguous fp32 (B,) device tensor receiving the loss.
        cond_mask (random_imp): the batch's (B,) condition-frame bitmasks -- the *_pose strategies take each window's
        ground-truth corrupt frames from it (mcd_aggregate_view)."""
        B, S = loss_all.shape
        # the C ABI takes dense (B,S) / (B,S,C,Tx,V) tensors: views with other strides (e.g. a transposed (S,B) stack) are copied
        loss_all = _f32c(loss_all, self.device)
        if poses_all is not None:
            poses_all = _f32c(poses_all, self.device)
        name, q = _aggregation_of(strategy, [a for a in _lib.AGGR if a != "all"], f"Unknown aggregation strategy {strategy}")
        cfg = self._score_cfg(B, S, int(noise_steps), loss_fn)
        needs_data = name in ("mean_pose", "median_pose")
        if torch.is_tensor(data):
            data = _f32c(data, self.device)
        elif needs_data:
            raise ValueError("the *_pose aggregation strategies need the materialised (B,C,T,V) windows")
        else:
            data = None
        out = _out_vector(out, B, self.device)
        gives_pose = name in ("best", "worst", "mean_pose", "median_pose")
        pose = None
        if gives_pose and want_pose and poses_all is not None:
            pose = torch.empty(poses_all.shape[0], *poses_all.shape[2:], device=self.device, dtype=torch.float32)
        if cond_mask is not None:
            cond_mask = _i32c(cond_mask, self.device)
            if cond_mask.numel() != B:
                raise ValueError(f"cond_mask must have {B} entries")
        view = _window_view(None, cond_mask) if cond_mask is not None else None      # (no mask: a null view, cfg's corrupt_idx)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_aggregate_view(C.byref(cfg), self.num_coords, self.n_joints, _lib.AGGR[name], C.c_float(q),
                                                 _ptr(loss_all), _ptr(poses_all), _ptr(data), C.byref(view) if view is not None else None,
                                                 _ptr(out), _ptr(pose), _stream()))
        return pose, out


class HipScorer(_Scorer):
    """One packed model on one GPU.

    state_dict: the reference's Lightning-checkpoint keys ('model.*', 'condition_encoder.*') -> tensors.
    strategy: canonical conditioning strategy ('inject' | 'concat' | 'no_condition' | 'inbetween_imp').
    cond_channels: output channels of the 'AE' / 'E' condition encoder's layers; cond_unet: 'E_unet' encoder instead.
    """

    _OPTIONS, _SET_OPTION, _FREE = _lib.OPT, "mcd_set_option", "mcd_free_weights"
    _step_table = staticmethod(step_table)

    def __init__(self, state_dict: Dict[str, torch.Tensor], *, strategy: str, seg_len: int, cond_idx: Sequence[int],
                 corrupt_idx: Sequence[int], cond_channels: Sequence[int] = (), cond_unet: bool = False,
                 num_coords: int = 2, n_joints: int = 17, emb_dim: int = 16, device=None,
                 options: Optional[Dict[str, int]] = None):
        self._init_model(seg_len, cond_idx, corrupt_idx, num_coords, n_joints, emb_dim)
        _need_gpu()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.strategy = strategy
        self.t_cond = len(self.cond_idx) if strategy == "inject" else 0
        self.t_unet = len(self.corrupt_idx) + (len(self.cond_idx) if strategy in ("concat", "inbetween_imp", "random_imp") else 0)
        cfg = self._model_cfg(strategy, self.t_unet, self.t_cond, cond_channels, cond_unet)
        arr, n, keep = _pack_tensors(state_dict)
        handle = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_pack_weights(arr, n, C.byref(cfg), idx, C.byref(handle)))
        del keep
        self._h = handle
        self._set_options(options)

    def plan_split(self, n_windows: int, n_samples: int, noise_steps: int) -> int:
        """How a scoring call of this size is cut into workgroups (mcd_plan_split): 1 = ONE launch (a workgroup runs all samples
        of its windows, condition encoder and aggregation inside), n_samples = one trajectory per workgroup + the encoder and
        the aggregation as their own launches, 0 = not on score_kernel (13 .. 32 U-Net frames: the slab-tiled kernel; or 'generic_unet')."""
        cfg = self._score_cfg(int(n_windows), int(n_samples), int(noise_steps), "smooth_l1")
        with torch.cuda.device(self.device):
            r = int(self.L.mcd_plan_split(self._h, C.byref(cfg)))
        if r < 0:
            _lib.check(r)
        return r

    # ------------------------------------------------------------------ entry points
    def cond_encode(self, cond_data: torch.Tensor) -> torch.Tensor:
        if self.strategy != "inject":
            raise ValueError("this model has no condition encoder")
        self._check_shape("cond_data", cond_data, (self.num_coords, self.t_cond, self.n_joints))
        x = _f32c(cond_data, self.device)
        out = torch.empty(x.shape[0], self.emb_dim, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_cond_encode(self._h, _ptr(x), x.shape[0], _ptr(out), _stream()))
        return out

    def unet_forward(self, x: torch.Tensor, t: int, cond: Optional[torch.Tensor], noise_steps: Optional[int] = None) -> torch.Tensor:
        self._check_shape("x", x, (self.num_coords, self.t_unet, self.n_joints))
        if cond is not None:
            self._check_shape("cond", cond, (self.emb_dim,))
            if cond.shape[0] != x.shape[0]:
                raise ValueError(f"cond has {cond.shape[0]} rows, x has {x.shape[0]} windows")
        x = _f32c(x, self.device)
        cond = None if cond is None else _f32c(cond, self.device)
        tab = self.table(noise_steps if noise_steps is not None else max(int(t) + 1, 2))
        out = torch.empty_like(x)
        with torch.cuda.device(self.device):
            ws = self._pass_workspace(x.shape[0])
            _lib.check(self.L.mcd_unet_forward(self._h, _ptr(x), _ptr(cond), _ptr(tab), int(t), x.shape[0], _ptr(out), _ptr(ws), _stream()))
        return out

    def _pass_workspace(self, n_windows: int) -> Optional[torch.Tensor]:
        """Scratch of the single-pass entries (mcd_pass_workspace_bytes): the slab-tiled kernel's activation slabs; None for
        1 .. 12 U-Net frames.  Call inside `torch.cuda.device(self.device)`."""
        nbytes = int(self.L.mcd_pass_workspace_bytes(self._h, int(n_windows)))
        return torch.empty(nbytes, device=self.device, dtype=torch.uint8) if nbytes > 0 else None

    def score(self, data, *, n_samples: int, noise_steps: int, noise: Optional[torch.Tensor] = None,
              seed: int = 0, first_window_id: int = 0, loss_fn: str = "smooth_l1", want_poses: bool = False,
              cond_mask: Optional[torch.Tensor] = None, want_maps: bool = False):
        """data (B,C,T,V) tensor, or a mocodad_amd.data.windows.WindowBatch (windows read in place from trajectory
        buffers, test-time transform applied on load) -> (loss (B,S), poses (B,S,C,Tx,V) | None).
        cond_mask (random_imp only): (B,) int32, bit t set = frame t of the window conditions.
        want_maps: a third result, the per-sample error maps E (B,S,Tx,V) (mcd_error_maps, MCD_AGGR_ALL): one more small launch
        behind the scoring call, on the poses it wrote (into the scorer's own per-stream buffer unless want_poses).
        Asynchronous on the current stream."""
        _, loss, poses, maps = self._score(data, n_samples, noise_steps, noise, seed, first_window_id, loss_fn, want_poses, cond_mask,
                                           aggregation=None, want_all=True, out=None, want_maps=want_maps)
        return (loss, poses, maps) if want_maps else (loss, poses)

    def score_fused(self, data, *, n_samples: int, noise_steps: int, aggregation: str = "best", noise: Optional[torch.Tensor] = None,
                    seed: int = 0, first_window_id: int = 0, loss_fn: str = "smooth_l1", want_all: bool = False, want_poses: bool = False,
                    cond_mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, want_maps: bool = False):
        """`score` + the loss-based aggregation over the samples ('best' | 'worst' | 'mean' | 'median' | 'quantile:q') in one
        call -- one kernel launch whenever the workgroups own whole windows (mcd_score_fused).
        -> (aggregated loss (B,), loss (B,S) | None, poses | None).  out: optional preallocated (B,) result.
        want_maps: a fourth result, the error maps M (B,Tx,V) under the aggregation (mean_{t,v} M[b] = loss[b] up to rounding;
        mcd_error_maps): the call then also writes the per-sample losses and the poses (into the scorer's own per-stream buffers
        unless asked for) and one small launch follows it."""
        r = self._score(data, n_samples, noise_steps, noise, seed, first_window_id, loss_fn, want_poses, cond_mask,
                        aggregation=aggregation, want_all=want_all, out=out, want_maps=want_maps)
        return r if want_maps else r[:3]

    def _score(self, data, n_samples, noise_steps, noise, seed, first_window_id, loss_fn, want_poses, cond_mask, *, aggregation,
               want_all, out, want_maps=False):
        if (cond_mask is not None) != (self.strategy == "random_imp"):
            raise ValueError("cond_mask is required by, and only valid for, the random_imp strategy")
        if cond_mask is not None:
            cond_mask = cond_mask.to(self.device, torch.int32).contiguous()
        data, view, B, keep = self._windows(data, cond_mask)
        S = int(n_samples)
        Tx = len(self.corrupt_idx)
        cfg = self._score_cfg(B, S, int(noise_steps), loss_fn)
        loss = torch.empty(B, S, device=self.device, dtype=torch.float32) if want_all else None
        poses = torch.empty(B, S, self.num_coords, Tx, self.n_joints, device=self.device, dtype=torch.float32) if want_poses else None
        if noise is not None:
            noise = _f32c(noise, self.device)
            exp = (S, max(noise_steps - 1, 1), B, self.num_coords, Tx, self.n_joints)
            if tuple(noise.shape) != exp:
                raise ValueError(f"noise must have shape {exp}, got {tuple(noise.shape)}")
        agg = None
        if aggregation is not None:
            name, q = _aggregation_of(aggregation, LOSS_AGGREGATIONS,
                                      f"score_fused aggregates losses (best, worst, mean, median, quantile:q), not {aggregation!r}")
            agg = _out_vector(out, B, self.device)
        need = int(self.L.mcd_score_workspace_bytes(self._h, C.byref(cfg)))
        maps = None
        with torch.cuda.device(self.device):
            # the maps launch reads the poses and (to select samples) the per-sample losses: the scoring call writes them into the
            # scorer's own buffers where the caller did not ask for them
            loss_w, poses_w = loss, poses
            if want_maps and B:
                if poses_w is None:
                    poses_w = self._scratch("poses", B * S * self.num_coords * Tx * self.n_joints).view(B, S, self.num_coords, Tx, self.n_joints)
                if loss_w is None:
                    loss_w = self._scratch("loss", B * S).view(B, S)
            common = (self._h, C.byref(cfg), _ptr(data), C.byref(view) if view is not None else None, _ptr(noise),
                      _seed64(seed), C.c_int64(first_window_id), _ptr(self.table(noise_steps)), _ptr(self._workspace(need)))
            if aggregation is None:
                _lib.check(self.L.mcd_score_view(*common, _ptr(loss_w), _ptr(poses_w), _stream()))
            else:
                _lib.check(self.L.mcd_score_fused(*common, _lib.AGGR[name], C.c_float(q), _ptr(agg), _ptr(loss_w), _ptr(poses_w), _stream()))
            if want_maps:
                mname, mq = ("all", 0.0) if aggregation is None else (name, q)
                if B:
                    maps = self._maps_launch(data, view, B, S, mname, mq, loss_w, poses_w, loss_fn)
                else:
                    maps = torch.empty((0, S, Tx, self.n_joints) if mname == "all" else (0, Tx, self.n_joints), device=self.device)
        del keep
        return agg, loss, poses, maps

    # stage ids of mcd_layer_forward: (Cin, Vin, Cout, Vout)
    _STAGES = {0: (2, 17, 16, 17), 1: (16, 17, 32, 17), 2: (32, 17, 32, 17), 3: (32, 12, 64, 12), 4: (64, 12, 64, 12),
               5: (64, 10, 128, 10), 6: (128, 10, 64, 10), 7: (64, 12, 64, 12), 8: (64, 12, 32, 12), 9: (32, 17, 32, 17),
               10: (32, 17, 2, 17), 11: (32, 17, 32, 12), 12: (64, 12, 64, 10), 13: (64, 10, 64, 12), 14: (32, 12, 32, 17)}

    # the fused (joint resampler + layer) stages of the slab-tiled kernel (13 .. 32 U-Net frames): the stage's input is the
    # RESAMPLER's input (Cin, Vin); the skip tensor of stages 7 / 9 has the layer's own (Cin, V)
    _FUSED_IN = {3: (32, 17), 5: (64, 12), 7: (64, 10), 9: (32, 12)}

    def layer_forward(self, stage: int, x: torch.Tensor, emb: torch.Tensor, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
        """TEST ENTRY: one U-Net stage alone (0..10 ST-GCN layers, 11..14 down1/down2/up3/up2), x (B,Cin,T,Vin),
        emb (B,emb_dim) -> (B,Cout,T,Vout).  13 .. 32 U-Net frames (slab-tiled kernel): stages 3, 5, 7, 9 are joint resampler +
        layer (x = the resampler's input; `skip` = d2 / d1 for stages 7 / 9), stages 11..14 do not exist on their own."""
        cin, vin, cout, vout = self._STAGES[int(stage)]
        tiled = self.t_unet > 12
        if tiled and int(stage) in self._FUSED_IN:
            lcin, lvin = cin, vin
            cin, vin = self._FUSED_IN[int(stage)]
            if skip is not None:
                self._check_shape("skip", skip, (lcin, self.t_unet, lvin))
                skip = _f32c(skip, self.device)
        elif skip is not None:
            raise ValueError("skip: only the fused stages 7 and 9 of the slab-tiled kernel (13 .. 32 U-Net frames) take one")
        self._check_shape("x", x, (cin, self.t_unet, vin))
        self._check_shape("emb", emb, (self.emb_dim,))
        x, emb = _f32c(x, self.device), _f32c(emb, self.device)
        out = torch.empty(x.shape[0], cout, self.t_unet, vout, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            ws = self._pass_workspace(x.shape[0])
            _lib.check(self.L.mcd_layer_forward(self._h, int(stage), _ptr(x), _ptr(skip), _ptr(emb), x.shape[0], _ptr(out), _ptr(ws), _stream()))
        return out

    def philox_noise(self, n_windows: int, *, n_samples: int, noise_steps: int, seed: int = 0, first_window_id: int = 0) -> torch.Tensor:
        """The noise tensor (S, max(ns-1,1), B, C, Tx, V) the perf mode of `score` draws in-kernel for these keys."""
        S, K, Tx = int(n_samples), max(int(noise_steps) - 1, 1), len(self.corrupt_idx)
        out = torch.empty(S, K, int(n_windows), self.num_coords, Tx, self.n_joints, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_philox_noise(_seed64(seed), C.c_int64(first_window_id), int(n_windows), S,
                                               int(noise_steps), Tx, _ptr(out), _stream()))
        return out

    def random_imp_masks(self, n_windows: int, seed: int = 0, first_window_id: int = 0) -> torch.Tensor:
        """'random_imp' condition-frame sets drawn on the device (mcd_random_imp_masks) -> (n_windows,) int32 bitmasks, keyed by
        (seed, global window id) like the perf-mode noise: no host work per batch.  Asynchronous on the current stream."""
        if self.strategy != "random_imp":
            raise ValueError("random_imp_masks: only the random_imp strategy draws per-window frame sets")
        n = int(n_windows)
        if n < 0:
            raise ValueError("n_windows must be >= 0")
        out = torch.empty(n, device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_random_imp_masks(_seed64(seed), C.c_int64(first_window_id), n, self.seg_len,
                                                   len(self.cond_idx), _ptr(out), _stream()))
        return out

    def scatter_max(self, scores: torch.Tensor, frames: torch.Tensor, row: torch.Tensor, n_rows: int, n_frames: int) -> torch.Tensor:
        scores, frames, row = _f32c(scores, self.device), _i32c(frames, self.device), _i32c(row, self.device)
        out = torch.empty(n_rows, n_frames, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_scatter_max(_ptr(scores), _ptr(frames), _ptr(row), scores.numel(), frames.shape[1],
                                              n_rows, n_frames, _ptr(out), _stream()))
        return out


class _LatentHandle(_Scorer):
    """What the two kinds of latent handle share: the library entries, the step table, and the packing of a state_dict -- the
    model configuration ('inject' only), the device choice, the call of the subclass's pack entry _PACK with its own arguments
    (_pack_args, between the configuration and the device index)."""

    _OPTIONS, _SET_OPTION, _FREE = _lib.LATENT_OPT, "mcd_latent_set_option", "mcd_free_latent_weights"
    _step_table = staticmethod(latent_step_table)
    _PACK = ""

    def __init__(self, state_dict: Dict[str, torch.Tensor], *, seg_len: int, cond_idx: Sequence[int], corrupt_idx: Sequence[int],
                 cond_channels: Sequence[int] = (), latent_dim: int, cond_unet: bool = False, num_coords: int = 2, n_joints: int = 17,
                 emb_dim: int = 16, device=None, options: Optional[Dict[str, int]] = None):
        self._init_model(seg_len, cond_idx, corrupt_idx, num_coords, n_joints, emb_dim)
        self.latent_dim = int(latent_dim)
        if len(cond_channels) > _lib.MCD_MAX_COND_LAYERS:
            raise ValueError(f"at most {_lib.MCD_MAX_COND_LAYERS} condition-encoder layers")
        cfg = self._model_cfg("inject", len(self.corrupt_idx), len(self.cond_idx), cond_channels, cond_unet)
        arr, n, keep = _pack_tensors(state_dict)
        # sizes and tensor names are checked by the library before it touches a device: those errors need no GPU
        have_gpu = torch.cuda.is_available()
        self.device = torch.device(device if device is not None else (f"cuda:{torch.cuda.current_device()}" if have_gpu else "cuda:0"))
        idx = self.device.index if self.device.index is not None else 0
        handle = C.c_void_p()
        _lib.check(getattr(self.L, self._PACK)(arr, n, C.byref(cfg), *self._pack_args(), idx, C.byref(handle)))
        del keep
        self._h = handle
        self._set_options(options)


class LatentScorer(_LatentHandle):
    """One packed MoCoDADlatent model (stage 'diffusion') on one GPU: the mcd_latent_* entry points.

    state_dict: the reference's keys ('model.*' without an up path, 'condition_encoder.*', 'denoiser.*').
    cond_channels: output channels of the 'AE' / 'E' condition encoder's layers; cond_unet: the 'E_unet' encoder instead.
    latent_dim / hidden_sizes: latent_embedding_dim and the denoiser's layer widths (the last equals latent_dim).
    3 or 5 .. 12 corrupt frames, 1 .. 12 condition frames (mcd_pack_latent_weights).  At 5 .. 12 corrupt frames a scoring call is
    four launches -- condition encoder, encode, the projection onto the latent (to_time_dim over all windows), chain -- and the
    workspace also holds the encoder's last activation (n_windows x 640 x corrupt frames floats); `encode`, `score` and the
    workspace size are used the same way."""

    _PACK = "mcd_pack_latent_weights"

    def __init__(self, state_dict: Dict[str, torch.Tensor], *, hidden_sizes: Sequence[int], **model):
        self.hidden_sizes = [int(h) for h in hidden_sizes]
        super().__init__(state_dict, **model)

    def _pack_args(self):
        lcfg = _lib.LatentCfg()
        lcfg.latent_dim, lcfg.n_layers = self.latent_dim, len(self.hidden_sizes)
        for i, h in enumerate(self.hidden_sizes[:8]):       # (more than 8 layers: the library refuses n_layers)
            lcfg.hidden[i] = h
        return [C.byref(lcfg)]

    def encode(self, data, *, noise_steps: int = 2) -> Tuple[torch.Tensor, torch.Tensor]:
        """windows -> (cond_emb (B,16), z0 (B,D)): condition encoder + down path at t = -1 + to_time_dim (mcd_latent_encode)."""
        data, view, B, keep = self._windows(data)
        cond = torch.empty(B, self.emb_dim, device=self.device, dtype=torch.float32)
        z0 = torch.empty(B, self.latent_dim, device=self.device, dtype=torch.float32)
        cfg = self._score_cfg(B, 1, int(noise_steps))
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_latent_encode(self._h, C.byref(cfg), _ptr(data), C.byref(view) if view is not None else None,
                                                _ptr(self.table(int(noise_steps))), _ptr(cond), _ptr(z0), _stream()))
        del keep
        return cond, z0

    def denoise(self, x: torch.Tensor, t: int, cond: torch.Tensor, noise_steps: Optional[int] = None) -> torch.Tensor:
        """TEST ENTRY: Denoiser.forward for rows x (N,D), cond (N,16) at step t -> (N,D)."""
        if x.dim() != 2 or x.shape[1] != self.latent_dim:
            raise ValueError(f"x must have shape (N, {self.latent_dim}), got {tuple(x.shape)}")
        if cond.dim() != 2 or tuple(cond.shape) != (x.shape[0], self.emb_dim):
            raise ValueError(f"cond must have shape ({x.shape[0]}, {self.emb_dim}), got {tuple(cond.shape)}")
        if int(t) < 0:
            raise ValueError("t must be >= 0")
        x, cond = _f32c(x, self.device), _f32c(cond, self.device)
        out = torch.empty_like(x)
        tab = self.table(noise_steps if noise_steps is not None else max(int(t) + 1, 2))
        if int(t) >= tab.shape[0] - 1:
            raise ValueError(f"t = {t} is outside the {tab.shape[0] - 1} steps of the table")
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_latent_denoise(self._h, _ptr(x), _ptr(cond), _ptr(tab), int(t), x.shape[0], _ptr(out), _stream()))
        return out

    def score(self, data, *, n_samples: int, noise_steps: int, aggregation: str = "all", noise: Optional[torch.Tensor] = None,
              seed: int = 0, first_window_id: int = 0, loss_fn: str = "smooth_l1", want_all: bool = False, want_latents: bool = False,
              want_code: bool = False, out: Optional[torch.Tensor] = None, want_cond: bool = False):
        """One MoCoDADlatent.forward (mcd_latent_score) -> (loss_agg (B,) | None, loss_all (B,S) | None, latent_all (B,S,D) | None,
        latent_code (B,D) | None).  aggregation: 'all' (per-sample losses only) or best | worst | mean | median | quantile:q.
        noise: (S, max(ns-1,1), B, D) replacing the in-kernel Philox stream.  out: optional preallocated (B,) tensor the
        aggregated losses are written into (it is then the first result).  want_cond: a fifth result, cond_emb (B,16) as the call
        computed it -- a view of the head of this stream's workspace (where mcd_latent_score leaves it), valid until the scorer's
        next call on the stream.  Asynchronous on the current stream."""
        data, view, B, keep = self._windows(data)
        S, ns, D = int(n_samples), int(noise_steps), self.latent_dim
        if S < 1 or ns < 2:
            raise ValueError("need n_samples >= 1 and noise_steps >= 2")
        name, q = _aggregation_of(aggregation, ("all",) + LOSS_AGGREGATIONS,
                                  f"the latent scoring call aggregates losses (all, best, worst, mean, median, quantile:q), not {aggregation!r}")
        if noise is not None:
            noise = _f32c(noise, self.device)
            exp = (S, max(ns - 1, 1), B, D)
            if tuple(noise.shape) != exp:
                raise ValueError(f"noise must have shape {exp}, got {tuple(noise.shape)}")
        dev = self.device
        if out is not None and name == "all":
            raise ValueError("out takes the aggregated losses: not valid with aggregation 'all'")
        agg = None if name == "all" else _out_vector(out, B, dev)
        loss = torch.empty(B, S, device=dev, dtype=torch.float32) if (want_all or name == "all") else None
        lat = torch.empty(B, S, D, device=dev, dtype=torch.float32) if want_latents else None
        code = torch.empty(B, D, device=dev, dtype=torch.float32) if want_code else None
        cfg = self._score_cfg(B, S, ns, loss_fn)
        with torch.cuda.device(dev):
            ws = self._workspace(int(self.L.mcd_latent_workspace_bytes(self._h, B)))
            if B:
                _lib.check(self.L.mcd_latent_score(self._h, C.byref(cfg), _ptr(data), C.byref(view) if view is not None else None,
                                                   _ptr(noise), _seed64(seed), C.c_int64(first_window_id),
                                                   _ptr(self.table(ns)), _ptr(ws), _lib.AGGR[name], C.c_float(q), _ptr(agg), _ptr(loss),
                                                   _ptr(lat), _ptr(code), _stream()))
        del keep
        if want_cond:
            return agg, loss, lat, code, ws[:B * self.emb_dim * 4].view(torch.float32).view(B, self.emb_dim)
        return agg, loss, lat, code

    def philox_noise(self, n_windows: int, *, n_samples: int, noise_steps: int, seed: int = 0, first_window_id: int = 0) -> torch.Tensor:
        """The draws (S, max(ns-1,1), B, D) the perf mode of `score` makes in-kernel for these keys."""
        S, K = int(n_samples), max(int(noise_steps) - 1, 1)
        out = torch.empty(S, K, int(n_windows), self.latent_dim, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_latent_philox_noise(_seed64(seed), C.c_int64(first_window_id), int(n_windows), S,
                                                      int(noise_steps), self.latent_dim, _ptr(out), _stream()))
        return out


class LatentReconstructor(_LatentHandle):
    """One packed MoCoDADlatent model of stage 'pretrain' -- the bottleneck autoencoder -- on one GPU: mcd_pack_latent_ae_weights
    and mcd_latent_reconstruct.

    state_dict: the reference's keys ('model.*' with the up path and rev_to_time_dim, 'condition_encoder.*'; no 'denoiser.*').
    The other arguments are LatentScorer's without hidden_sizes.  3 or 5 .. 12 corrupt frames, 1 .. 12 condition frames.  A call is
    [condition encoder] -> encode -> [project] -> unproject -> decode; the workspace holds cond_emb, z0 and one
    n_windows x 640 x corrupt-frames region (the encoder's last activation, then the decoder's first).  decode_samples decodes the
    (B,S,D) latents another model generated for the windows -- the diffusion stage's, whose decoder this handle is
    (MoCoDADlatent.load_decoder) -- in one call; aggregate / error_maps / joint_scatter_max of the base class take its results."""

    _PACK = "mcd_pack_latent_ae_weights"

    def _pack_args(self):
        return [self.latent_dim]

    def reconstruct(self, data, z: Optional[torch.Tensor] = None, *, want_pose: bool = True, want_code: bool = False,
                    loss_fn: str = "smooth_l1", noise_steps: int = 2):
        """One pass of the autoencoder (mcd_latent_reconstruct) -> (pose (B,2,t_unet,17) | None, loss (B,), cond_emb (B,16),
        z0 (B,D) | None).  z: (B,D) latents to decode in place of the windows' own codes (with the windows' own skips and
        condition); z0 is the windows' own code either way.  loss: mean loss_fn(pose, corrupt frames) per window.  noise_steps
        only sizes the step table, whose last row holds the constant time step -1.  Asynchronous on the current stream."""
        data, view, B, keep = self._windows(data)
        D, dev = self.latent_dim, self.device
        if z is not None:
            if z.dim() != 2 or tuple(z.shape) != (B, D):
                raise ValueError(f"z must have shape ({B}, {D}), got {tuple(z.shape)}")
            z = _f32c(z, dev)
        pose = torch.empty(B, self.num_coords, len(self.corrupt_idx), self.n_joints, device=dev, dtype=torch.float32) if want_pose else None
        loss = torch.empty(B, device=dev, dtype=torch.float32)
        cond = torch.empty(B, self.emb_dim, device=dev, dtype=torch.float32)
        code = torch.empty(B, D, device=dev, dtype=torch.float32) if want_code else None
        cfg = self._score_cfg(B, 1, int(noise_steps), loss_fn)
        with torch.cuda.device(dev):
            ws = self._workspace(int(self.L.mcd_latent_workspace_bytes(self._h, B)))
            if B:
                _lib.check(self.L.mcd_latent_reconstruct(self._h, C.byref(cfg), _ptr(data), C.byref(view) if view is not None else None,
                                                         _ptr(self.table(int(noise_steps))), _ptr(ws), _ptr(z), _ptr(pose), _ptr(loss),
                                                         _ptr(cond), _ptr(code), _stream()))
        del keep
        return pose, loss, cond, code

    def decode_samples(self, data, latents: torch.Tensor, cond_emb: Optional[torch.Tensor] = None, *, want_poses: bool = True,
                       loss_fn: str = "smooth_l1", noise_steps: int = 2):
        """The decoder on all generated latents of each window (mcd_latent_decode_samples): latents (B,S,D) -- e.g. latent_all of
        LatentScorer.score -- -> (pose_all (B,S,2,t_unet,17) | None, loss_all (B,S)): sample s of window b decoded with the window's
        own skips and condition, and its mean loss_fn against the window's corrupt frames; column s is bit for bit
        reconstruct(data, z=latents[:, s]).  cond_emb: (B,16) as LatentScorer.encode / score computed it for these windows (None:
        this handle's condition encoder runs in front).  The results have the layout of HipScorer.score's: `aggregate` and
        `error_maps` take them.  Asynchronous on the current stream."""
        data, view, B, keep = self._windows(data)
        D, dev = self.latent_dim, self.device
        if latents.dim() != 3 or latents.shape[0] != B or latents.shape[1] < 1 or latents.shape[2] != D:
            raise ValueError(f"latents must have shape ({B}, S >= 1, {D}), got {tuple(latents.shape)}")
        latents = _f32c(latents, dev)
        S = int(latents.shape[1])
        if cond_emb is not None:
            if tuple(cond_emb.shape) != (B, self.emb_dim):
                raise ValueError(f"cond_emb must have shape ({B}, {self.emb_dim}), got {tuple(cond_emb.shape)}")
            cond_emb = _f32c(cond_emb, dev)
        poses = torch.empty(B, S, self.num_coords, len(self.corrupt_idx), self.n_joints, device=dev, dtype=torch.float32) if want_poses else None
        loss = torch.empty(B, S, device=dev, dtype=torch.float32)
        cfg = self._score_cfg(B, S, int(noise_steps), loss_fn)
        with torch.cuda.device(dev):
            ws = self._workspace(int(self.L.mcd_latent_decode_workspace_bytes(self._h, B, S)))
            if B:
                _lib.check(self.L.mcd_latent_decode_samples(self._h, C.byref(cfg), _ptr(data), C.byref(view) if view is not None else None,
                                                            _ptr(self.table(int(noise_steps))), _ptr(ws), _ptr(cond_emb), _ptr(latents),
                                                            _ptr(poses), _ptr(loss), _stream()))
        del keep
        return poses, loss


class LatentPoseScorer:
    """MoCoDADlatent scored in pose space in ONE library call (mcd_latent_score_pose) over two handles: a LatentScorer (the diffusion
    stage) and the LatentReconstructor that decodes its latents (MoCoDADlatent.load_decoder).  The call makes the launches of
    LatentScorer.score('all', want_latents) -> LatentReconstructor.decode_samples -> aggregate -> [error_maps] in that order, so
    every result is bit for bit theirs; cond_emb, the latents and whatever per-sample result nobody asked for stay in this object's
    per-stream workspace.  The results have HipScorer.score_fused's layout, and `corrupt_idx` / `_score_cfg` are the decoder
    handle's: a live stream drives this object exactly as it drives a HipScorer.  It owns no handle (the two scorers do)."""

    def __init__(self, scorer: "LatentScorer", decoder: "LatentReconstructor"):
        if not isinstance(scorer, LatentScorer) or not isinstance(decoder, LatentReconstructor):
            raise TypeError("LatentPoseScorer takes a LatentScorer (diffusion stage) and a LatentReconstructor (its decoder), in this order")
        for name in ("seg_len", "cond_idx", "corrupt_idx", "latent_dim", "device"):
            if getattr(scorer, name) != getattr(decoder, name):
                raise ValueError(f"LatentPoseScorer: the two handles differ in {name}: {getattr(scorer, name)} / {getattr(decoder, name)}")
        self.scorer, self.decoder = scorer, decoder
        self.L, self.device = scorer.L, scorer.device
        self.seg_len, self.latent_dim = scorer.seg_len, scorer.latent_dim
        self.num_coords, self.n_joints, self.emb_dim = decoder.num_coords, decoder.n_joints, decoder.emb_dim
        self._ws: Dict[int, torch.Tensor] = {}      # one workspace per stream, as _Scorer keeps them

    _workspace = _Scorer._workspace

    @property
    def corrupt_idx(self):
        return self.decoder.corrupt_idx

    @property
    def cond_idx(self):
        return self.decoder.cond_idx

    def _score_cfg(self, B: int, S: int, ns: int, loss_fn: str = "smooth_l1") -> "_lib.ScoreCfg":
        return self.decoder._score_cfg(B, S, ns, loss_fn)

    def philox_noise(self, n_windows: int, **kw) -> torch.Tensor:
        """The draws the perf mode of `score` makes in-kernel: LatentScorer.philox_noise."""
        return self.scorer.philox_noise(n_windows, **kw)

    def score(self, data, *, n_samples: int, noise_steps: int, aggregation: str = "best", noise: Optional[torch.Tensor] = None,
              seed: int = 0, first_window_id: int = 0, loss_fn: str = "smooth_l1", want_all: bool = False, want_poses: bool = False,
              want_maps: bool = False, out: Optional[torch.Tensor] = None, want_selected: bool = False, want_latents: bool = False):
        """data ((B,C,T,V) tensor or WindowBatch) -> (loss_agg (B,), loss_all (B,S) | None, poses_all (B,S,2,Tx,17) | None,
        maps (B,Tx,17) | None), as HipScorer.score_fused with want_maps returns them -- the losses taken on the decoded forecasts
        against the window's corrupt frames.  aggregation: best | worst | mean | median | quantile:q.  noise: (S, max(ns-1,1), B, D)
        replacing the in-kernel Philox draws of the chain.  out: optional preallocated (B,) result.  want_selected: a fifth result,
        the selected forecast (B,2,Tx,17) under best / worst (None under the others); want_latents: one more, the generated
        latents (B,S,D).  Asynchronous on the current stream."""
        data, view, B, keep = self.scorer._windows(data)
        S, ns, D, dev = int(n_samples), int(noise_steps), self.latent_dim, self.device
        if S < 1 or ns < 2:
            raise ValueError("need n_samples >= 1 and noise_steps >= 2")
        name, q = _aggregation_of(aggregation, LOSS_AGGREGATIONS,
                                  f"the pose-space scoring call aggregates losses (best, worst, mean, median, quantile:q), not {aggregation!r}")
        if noise is not None:
            noise = _f32c(noise, dev)
            exp = (S, max(ns - 1, 1), B, D)
            if tuple(noise.shape) != exp:
                raise ValueError(f"noise must have shape {exp}, got {tuple(noise.shape)}")
        Tx, C_, V = len(self.corrupt_idx), self.num_coords, self.n_joints
        agg = _out_vector(out, B, dev)
        loss = torch.empty(B, S, device=dev, dtype=torch.float32) if want_all else None
        poses = torch.empty(B, S, C_, Tx, V, device=dev, dtype=torch.float32) if want_poses else None
        maps = torch.empty(B, Tx, V, device=dev, dtype=torch.float32) if want_maps else None
        sel = torch.empty(B, C_, Tx, V, device=dev, dtype=torch.float32) if want_selected and name in ("best", "worst") else None
        lat = torch.empty(B, S, D, device=dev, dtype=torch.float32) if want_latents else None
        cfg = self._score_cfg(B, S, ns, loss_fn)
        with torch.cuda.device(dev):
            ws = self._workspace(int(self.L.mcd_latent_pose_workspace_bytes(self.scorer._h, self.decoder._h, B, S)))
            if B:
                _lib.check(self.L.mcd_latent_score_pose(self.scorer._h, self.decoder._h, C.byref(cfg), _ptr(data),
                                                        C.byref(view) if view is not None else None, _ptr(noise), _seed64(seed),
                                                        C.c_int64(first_window_id), _ptr(self.scorer.table(ns)), _ptr(ws), _lib.AGGR[name],
                                                        C.c_float(q), _ptr(agg), _ptr(loss), _ptr(poses), _ptr(sel), _ptr(maps), _ptr(lat),
                                                        _stream()))
        del keep
        res = (agg, loss, poses, maps)
        if want_selected:
            res += (sel,)
        if want_latents:
            res += (lat,)
        return res


def _scaler_stats(center, scale, dev) -> tuple:
    """(center, scale) as (34,) float64 device tensors (the precision sklearn's transform runs in), or (None, None)."""
    if (center is None) != (scale is None):
        raise ValueError("center and scale go together (both None = no robust scaling)")
    stats = []
    for name, a in (("center", center), ("scale", scale)):
        if a is None:
            return None, None
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.shape != (34,):
            raise ValueError(f"{name} must hold 34 features, got shape {a.shape}")
        stats.append(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev))
    return tuple(stats)


def _vid_res(vid_res: Sequence[float], need: str = "finite") -> tuple:
    """The image size as the fp32 values the kernels take; `need`: what the caller's error text asks for ('finite': the caller
    unpacks the pair, and another length fails there)."""
    res = tuple(float(np.float32(v)) for v in vid_res)
    if (len(res) != 2 and need != "finite") or (len(res) == 2 and not all(np.isfinite(res))):
        raise ValueError(f"vid_res must be {need}, got {tuple(vid_res)}")
    return res


def forecast_codes(method: str, spread: str, names: Tuple[str, str] = ("method", "spread_method"),
                   spreads: str = "'mean' or 'median'") -> Tuple[int, int]:
    """The names of a forecast method and spread -> their MCD_FORECAST_* codes; `names` and `spreads`: the caller's error text."""
    if method not in _lib.FORECAST:
        raise ValueError(f"{names[0]} must be one of {tuple(_lib.FORECAST)}, got {method!r}")
    if spread not in ("mean", "median"):
        raise ValueError(f"{names[1]} must be {spreads}, got {spread!r}")
    return _lib.FORECAST[method], _lib.FORECAST[spread]


def normalize_poses(raw, vid_res: Sequence[float], center=None, scale=None, *, device=None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dataset loader step (mcd_normalize_poses): raw (n_frames, 34) fp32 pose rows as read from the CSVs (x1,y1,...,x17,y17;
    host array or tensor on any device) -> (n_frames, 2, 17) fp32 on `device`: bounding-box-centre coordinates
    (utils/data.py:11-43,165-186) and, when center / scale (34,) are given, the RobustScaler transform (utils/data.py:350-359)
    with the fitted statistics in the CSV's interleaved feature order.  `out`: an (n_frames, 2, 17) fp32 device view to write
    into instead (e.g. a slice of a larger trajectory buffer)."""
    L = _lib.lib()
    _need_gpu()
    if (center is None) != (scale is None):
        raise ValueError("center and scale go together (both None = no robust scaling)")
    dev = torch.device(device if device is not None else (out.device if out is not None else f"cuda:{torch.cuda.current_device()}"))
    if torch.is_tensor(raw) and raw.device.type == "cuda":
        raw = raw.to(dev, torch.float32).contiguous()
        finite = (not raw.numel()) or bool(torch.isfinite(raw).all().item())
    else:
        raw_h = np.ascontiguousarray(raw.numpy() if torch.is_tensor(raw) else raw, dtype=np.float32)
        finite = bool(np.isfinite(raw_h).all())
        raw = None
    shape = tuple((raw if raw is not None else raw_h).shape)
    if len(shape) != 2 or shape[1] != 34:
        raise ValueError(f"raw pose rows must be (n_frames, 34) = x1,y1,...,x17,y17, got {shape}")
    if not finite:
        raise ValueError("raw pose rows hold NaN / inf values (the trajectory CSVs hold finite coordinates only)")
    w, h = _vid_res(vid_res)
    c, s = _scaler_stats(center, scale, dev)
    n = shape[0]
    if out is None:
        out = torch.empty(n, 2, 17, device=dev, dtype=torch.float32)
    elif out.shape != (n, 2, 17) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous (n_frames, 2, 17) fp32 tensor on the device")
    with torch.cuda.device(dev):
        if raw is None:
            raw = torch.from_numpy(raw_h).to(dev)
        _lib.check(L.mcd_normalize_poses(_ptr(raw), n, w, h, _ptr(c), _ptr(s), _ptr(out), _stream()))
    return out


def _call_device(device, *tensors) -> torch.device:
    """The device of a handle-free call: `device` when given, else that of the first of `tensors` on a GPU, else the current one."""
    if device is not None:
        return torch.device(device)
    for t in tensors:
        if t is not None and t.device.type == "cuda":
            return t.device
    _need_gpu()
    return torch.device(f"cuda:{torch.cuda.current_device()}")


def _caller_buffer(name: str, t: Optional[torch.Tensor], shape: Tuple[int, ...], dtype, dev) -> Optional[torch.Tensor]:
    """A caller's output buffer, checked (None: the wrapper allocates)."""
    if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev):
        raise ValueError(f"{name} must be a contiguous {tuple(shape)} {str(dtype).replace('torch.', '')} tensor on {dev}")
    return t


def forecast_assemble(poses: torch.Tensor, cell: torch.Tensor, n_cells: int, *, method: str = "median", spread_method: str = "mean",
                      max_cover: int = _lib.MCD_MAX_FRAMES, device=None, out=None,
                      workspace: Optional[torch.Tensor] = None, trans: Optional[torch.Tensor] = None,
                      inv_affine=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """mcd_forecast_assemble (utils/eval_utils.py:13-24, 37-72): the selected forecasts of overlapping windows, poses (N,2,Tx,17),
    collapsed into one pose per output cell; cell (N,Tx) int32 names the cell of every forecast frame, a value outside
    [0, n_cells) means "ignore".  method: 'unique' (the lowest window index) | 'mean' | 'median'; spread_method: 'mean' | 'median'
    of the 34 per-feature standard deviations over the windows covering the cell; max_cover 1 .. 32: pairs a cell's list holds.
    -> (pose (n_cells, 34) fp32 interleaved x1,y1,...,x17,y17, count (n_cells,) int32, spread (n_cells,) fp32); a cell nobody
    forecasts is 0 with count 0, one with more than max_cover pairs is NaN with its true count.  out: the caller's three buffers
    instead of new ones; workspace: the caller's int32 scratch of at least n_cells * max_cover words.
    trans (N,) integer + inv_affine (n_transform, 6) float64 (utils.transforms.inverse_affine_table): mcd_forecast_assemble_view --
    the forecast of window i is first mapped back through row trans[i] of the inverse table, so the windows of every test-time
    transform forecast a cell in the coordinates of transform 0; a window whose transform is outside the table is ignored;
    max_cover 1 .. 64 then.  Both None (the default): mcd_forecast_assemble.  Asynchronous on the current
    stream; arguments are checked before anything touches the device."""
    codes = forecast_codes(method, spread_method)
    max_cover, n_cells = int(max_cover), int(n_cells)
    if (trans is None) != (inv_affine is None):
        raise ValueError("trans and inv_affine go together (both None = no transforms)")
    cover_max = _lib.MCD_MAX_FRAMES if trans is None else _lib.MCD_FORECAST_VIEW_COVER
    if not 1 <= max_cover <= cover_max:
        raise ValueError(f"max_cover must be in 1 .. {cover_max}, got {max_cover}")
    if n_cells < 0:
        raise ValueError(f"n_cells must be >= 0, got {n_cells}")
    if poses.dim() != 4 or poses.shape[1] != 2 or poses.shape[3] != 17 or not 1 <= poses.shape[2] <= _lib.MCD_MAX_FRAMES:
        raise ValueError(f"poses must have shape (N, 2, Tx, 17) with 1 <= Tx <= {_lib.MCD_MAX_FRAMES}, got {tuple(poses.shape)}")
    N, Tx = int(poses.shape[0]), int(poses.shape[2])
    if tuple(cell.shape) != (N, Tx) or cell.dtype.is_floating_point:
        raise ValueError(f"cell must be an integer ({N}, {Tx}) tensor, got {tuple(cell.shape)} {cell.dtype}")
    if N * Tx > 2**31 - 1:
        raise ValueError("N x Tx exceeds 2^31 - 1: assemble in smaller batches")
    if trans is not None:
        if tuple(trans.shape) != (N,) or trans.dtype.is_floating_point:
            raise ValueError(f"trans must be an integer ({N},) tensor, got {tuple(trans.shape)} {trans.dtype}")
        if not torch.is_tensor(inv_affine):      # (a list through torch.as_tensor would pass through float32)
            inv_affine = torch.from_numpy(np.ascontiguousarray(inv_affine, dtype=np.float64))
        if inv_affine.dim() != 2 or inv_affine.shape[0] < 1 or inv_affine.shape[1] != 6:
            raise ValueError(f"inv_affine must be (n_transform, 6) with n_transform >= 1, got {tuple(inv_affine.shape)}")
    dev = _call_device(device, poses)
    if out is not None and len(out) != 3:
        raise ValueError("out must be the three buffers (pose, count, spread)")
    o_pose, o_count, o_spread = out if out is not None else (None, None, None)
    o_pose = _caller_buffer("out[0] (pose)", o_pose, (n_cells, 34), torch.float32, dev)
    o_count = _caller_buffer("out[1] (count)", o_count, (n_cells,), torch.int32, dev)
    o_spread = _caller_buffer("out[2] (spread)", o_spread, (n_cells,), torch.float32, dev)
    if workspace is not None and (workspace.dtype != torch.int32 or not workspace.is_contiguous() or workspace.device != dev
                                  or workspace.numel() < n_cells * max_cover):
        raise ValueError(f"workspace must be a contiguous int32 tensor of at least n_cells x max_cover = {n_cells * max_cover} words on {dev}")
    L = _lib.lib()
    _need_gpu()
    poses, cell = _f32c(poses, dev), _i32c(cell, dev)
    with torch.cuda.device(dev):
        if o_pose is None:
            o_pose = torch.empty(n_cells, 34, device=dev, dtype=torch.float32)
        if o_count is None:
            o_count = torch.empty(n_cells, device=dev, dtype=torch.int32)
        if o_spread is None:
            o_spread = torch.empty(n_cells, device=dev, dtype=torch.float32)
        if workspace is None:
            workspace = torch.empty(max(n_cells * max_cover, 1), device=dev, dtype=torch.int32)
        if trans is None:
            _lib.check(L.mcd_forecast_assemble(_ptr(poses), _ptr(cell), N, Tx, n_cells, codes[0], codes[1], max_cover, _ptr(workspace),
                                               _ptr(o_pose), _ptr(o_count), _ptr(o_spread), _stream()))
        else:
            # (an empty tensor has no address, and a NULL trans would mean "no transforms": one word stands in, no window reads it)
            trans = _i32c(trans, dev) if N else torch.zeros(1, device=dev, dtype=torch.int32)
            inv = inv_affine.to(dev, torch.float64).contiguous()
            _lib.check(L.mcd_forecast_assemble_view(_ptr(poses), _ptr(cell), _ptr(trans), _ptr(inv), int(inv.shape[0]), N, Tx, n_cells,
                                                    codes[0], codes[1], max_cover, _ptr(workspace), _ptr(o_pose), _ptr(o_count),
                                                    _ptr(o_spread), _stream()))
    return o_pose, o_count, o_spread


def forecast_levels(levels, name: str = "levels") -> Tuple[float, ...]:
    """The quantile levels of a forecast fan as floats: 1 .. 8 (MCD_FORECAST_FAN_LEVELS) values in [0, 1], strictly ascending."""
    try:
        lv = tuple(float(q) for q in levels)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a sequence of numbers, got {levels!r}") from None
    if not 1 <= len(lv) <= _lib.MCD_FORECAST_FAN_LEVELS:
        raise ValueError(f"{name} must hold 1 .. {_lib.MCD_FORECAST_FAN_LEVELS} values, got {len(lv)}")
    if not all(0.0 <= q <= 1.0 for q in lv):
        raise ValueError(f"{name} must lie in [0, 1], got {lv}")
    if any(b <= a for a, b in zip(lv, lv[1:])):
        raise ValueError(f"{name} must be strictly ascending, got {lv}")
    return lv


def forecast_fan(poses_all: torch.Tensor, cell: torch.Tensor, n_cells: int, *, levels=(0.1, 0.5, 0.9), observed: Optional[torch.Tensor] = None,
                 max_cover: int = _lib.MCD_MAX_FRAMES, trans: Optional[torch.Tensor] = None, inv_affine=None, device=None, out=None,
                 workspace: Optional[torch.Tensor] = None):
    """mcd_forecast_fan: the distribution of ALL generated futures of a cell.  poses_all (N,S,2,Tx,17): every sample of every
    window (HipScorer.score's poses, forward(return_samples=True)); cell (N,Tx), max_cover, trans, inv_affine, workspace: as for
    forecast_assemble.  The value list of a cell's feature holds the S samples of each of its k covering pairs in ascending pair
    index, K = k * S values (at most 1024), mapped back when trans is given.  levels: 1 .. 8 quantile levels in [0, 1], strictly
    ascending.  observed (n_cells,2,17) fp32 in the trajectory buffer's frame-major layout (TrajectoryWindows.buffer viewed so), or
    None: no rank.
    -> (quant (n_levels, n_cells, 34) fp32, level-major, interleaved x1,y1,...; mean, std (n_cells, 34) fp32; rank (n_cells, 34)
    fp32 = (below + equal / 2) / K of the observed coordinate, or None; count (n_cells,) int32 = k).  A cell nobody forecasts is 0
    with count 0; one with k > max_cover or K > 1024 is NaN with its true count.  out: the caller's five buffers (the fourth None
    without `observed`) instead of new ones.  Asynchronous on the current stream; arguments are checked before anything touches the
    device."""
    lv = forecast_levels(levels)
    max_cover, n_cells = int(max_cover), int(n_cells)
    if (trans is None) != (inv_affine is None):
        raise ValueError("trans and inv_affine go together (both None = no transforms)")
    cover_max = _lib.MCD_MAX_FRAMES if trans is None else _lib.MCD_FORECAST_VIEW_COVER
    if not 1 <= max_cover <= cover_max:
        raise ValueError(f"max_cover must be in 1 .. {cover_max}, got {max_cover}")
    if n_cells < 0:
        raise ValueError(f"n_cells must be >= 0, got {n_cells}")
    if poses_all.dim() != 5 or poses_all.shape[1] < 1 or poses_all.shape[2] != 2 or poses_all.shape[4] != 17 \
            or not 1 <= poses_all.shape[3] <= _lib.MCD_MAX_FRAMES:
        raise ValueError(f"poses_all must have shape (N, S, 2, Tx, 17) with S >= 1 and 1 <= Tx <= {_lib.MCD_MAX_FRAMES}, got {tuple(poses_all.shape)}")
    N, S, Tx = int(poses_all.shape[0]), int(poses_all.shape[1]), int(poses_all.shape[3])
    if tuple(cell.shape) != (N, Tx) or cell.dtype.is_floating_point:
        raise ValueError(f"cell must be an integer ({N}, {Tx}) tensor, got {tuple(cell.shape)} {cell.dtype}")
    if N * Tx > 2**31 - 1:
        raise ValueError("N x Tx exceeds 2^31 - 1: assemble in smaller batches")
    if trans is not None:
        if tuple(trans.shape) != (N,) or trans.dtype.is_floating_point:
            raise ValueError(f"trans must be an integer ({N},) tensor, got {tuple(trans.shape)} {trans.dtype}")
        if not torch.is_tensor(inv_affine):      # (a list through torch.as_tensor would pass through float32)
            inv_affine = torch.from_numpy(np.ascontiguousarray(inv_affine, dtype=np.float64))
        if inv_affine.dim() != 2 or inv_affine.shape[0] < 1 or inv_affine.shape[1] != 6:
            raise ValueError(f"inv_affine must be (n_transform, 6) with n_transform >= 1, got {tuple(inv_affine.shape)}")
    if observed is not None and (tuple(observed.shape) != (n_cells, 2, 17) or observed.dtype != torch.float32):
        raise ValueError(f"observed must be a float32 ({n_cells}, 2, 17) tensor, got {tuple(observed.shape)} {observed.dtype}")
    dev = _call_device(device, poses_all)
    if out is not None and len(out) != 5:
        raise ValueError("out must be the five buffers (quant, mean, std, rank, count)")
    o_quant, o_mean, o_std, o_rank, o_count = out if out is not None else (None,) * 5
    if observed is None and o_rank is not None:
        raise ValueError("out[3] (rank) must be None without observed")
    o_quant = _caller_buffer("out[0] (quant)", o_quant, (len(lv), n_cells, 34), torch.float32, dev)
    o_mean = _caller_buffer("out[1] (mean)", o_mean, (n_cells, 34), torch.float32, dev)
    o_std = _caller_buffer("out[2] (std)", o_std, (n_cells, 34), torch.float32, dev)
    o_rank = _caller_buffer("out[3] (rank)", o_rank, (n_cells, 34), torch.float32, dev)
    o_count = _caller_buffer("out[4] (count)", o_count, (n_cells,), torch.int32, dev)
    if workspace is not None and (workspace.dtype != torch.int32 or not workspace.is_contiguous() or workspace.device != dev
                                  or workspace.numel() < n_cells * max_cover):
        raise ValueError(f"workspace must be a contiguous int32 tensor of at least n_cells x max_cover = {n_cells * max_cover} words on {dev}")
    L = _lib.lib()
    _need_gpu()
    poses_all, cell = _f32c(poses_all, dev), _i32c(cell, dev)
    c_levels = (C.c_double * len(lv))(*lv)
    with torch.cuda.device(dev):
        if o_quant is None:
            o_quant = torch.empty(len(lv), n_cells, 34, device=dev, dtype=torch.float32)
        if o_mean is None:
            o_mean = torch.empty(n_cells, 34, device=dev, dtype=torch.float32)
        if o_std is None:
            o_std = torch.empty(n_cells, 34, device=dev, dtype=torch.float32)
        if observed is not None:
            observed = _f32c(observed, dev)
            if o_rank is None:
                o_rank = torch.empty(n_cells, 34, device=dev, dtype=torch.float32)
        if o_count is None:
            o_count = torch.empty(n_cells, device=dev, dtype=torch.int32)
        if workspace is None:
            workspace = torch.empty(max(n_cells * max_cover, 1), device=dev, dtype=torch.int32)
        inv, n_t = None, 0
        if trans is not None:
            # (an empty tensor has no address, and a NULL trans would mean "no transforms": one word stands in, no window reads it)
            trans = _i32c(trans, dev) if N else torch.zeros(1, device=dev, dtype=torch.int32)
            inv = inv_affine.to(dev, torch.float64).contiguous()
            n_t = int(inv.shape[0])
        # (n_cells == 0: observed and rank are both empty, both without an address, and the entry returns before it reads a pointer)
        _lib.check(L.mcd_forecast_fan(_ptr(poses_all), _ptr(cell), _ptr(trans), _ptr(inv), n_t, N, S, Tx, n_cells, c_levels, len(lv),
                                      max_cover, _ptr(observed), _ptr(workspace), _ptr(o_quant), _ptr(o_mean), _ptr(o_std), _ptr(o_rank),
                                      _ptr(o_count), _stream()))
    return o_quant, o_mean, o_std, o_rank, o_count


def denormalize_poses(norm: torch.Tensor, raw, vid_res: Sequence[float], center=None, scale=None, count: Optional[torch.Tensor] = None, *,
                      device=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mcd_denormalize_poses, the inverse of normalize_poses: norm (n, 34) fp32 in the CSV's interleaved order (what
    forecast_assemble writes) -> (n, 34) fp32 image pixels in the bounding box of raw (n, 34), the observed CSV row of the same
    person and frame (host array or tensor; finite); center / scale (34,): the scaler statistics normalize_poses was given, or both
    None.  count (n,) int32: rows with count 0 come back all zero, the CSV's "missing".  out: an (n, 34) fp32 device buffer to
    write into.  Asynchronous on the current stream; arguments are checked before anything touches the device."""
    if (center is None) != (scale is None):
        raise ValueError("center and scale go together (both None = no robust scaling)")
    if norm.dim() != 2 or norm.shape[1] != 34:
        raise ValueError(f"norm must be (n, 34) = x1,y1,...,x17,y17, got {tuple(norm.shape)}")
    n = int(norm.shape[0])
    raw_t = raw if torch.is_tensor(raw) else torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32))
    if tuple(raw_t.shape) != (n, 34):
        raise ValueError(f"raw pose rows must be ({n}, 34) like norm, got {tuple(raw_t.shape)}")
    if raw_t.numel() and not bool(torch.isfinite(raw_t).all().item()):
        raise ValueError("raw pose rows hold NaN / inf values (the trajectory CSVs hold finite coordinates only)")
    if count is not None and (tuple(count.shape) != (n,) or count.dtype.is_floating_point):
        raise ValueError(f"count must be an integer ({n},) tensor, got {tuple(count.shape)} {count.dtype}")
    w, h = _vid_res(vid_res)
    for name, a in (("center", center), ("scale", scale)):
        if a is not None and tuple(np.shape(a) if not torch.is_tensor(a) else a.shape) != (34,):
            raise ValueError(f"{name} must hold 34 features, got shape {tuple(np.shape(a) if not torch.is_tensor(a) else a.shape)}")
    dev = _call_device(device, out, norm)
    out = _caller_buffer("out", out, (n, 34), torch.float32, dev)
    L = _lib.lib()
    _need_gpu()
    c, s = _scaler_stats(center, scale, dev)
    norm, raw_t = _f32c(norm, dev), _f32c(raw_t, dev)
    count = _i32c(count, dev) if count is not None else None
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(n, 34, device=dev, dtype=torch.float32)
        _lib.check(L.mcd_denormalize_poses(_ptr(norm), _ptr(raw_t), _ptr(count), n, w, h, _ptr(c), _ptr(s), _ptr(out), _stream()))
    return out


class StreamRings:
    """Device state of a live pose stream (mcd_stream_state_t) and the launches on it: flush, push_group and frame_scores_group
    per group of ticks (a single tick is a group of one); the host half -- which track owns which slot, row counts, frame
    ids -- is mocodad_amd.stream.TrackTable, the call that ties them together PoseStream.push / push_many.
      ring          flat (n_slots * 2 * ring_len * 34,) fp32: row r of slot s at positions r % L and r % L + L of its 2 L rows
      frame_scores  (n_slots, num_transform, ring_len) fp32 running maxima
    and, opt-in, the joint ring (joint_scores=True: mcd_stream_joint_state_t) and the forecast and observed rings (forecasts=(method,
    spread, n_corrupt): mcd_stream_forecast_state_t; forecast_group / forecast_flush).
    vid_res / center / scale: as for normalize_poses.  All calls are asynchronous on the current stream; one state is driven
    from one stream."""

    def __init__(self, n_slots: int, seg_len: int, ring_len: int, num_transform: int, vid_res: Sequence[float], center=None,
                 scale=None, *, device=None, joint_scores: bool = False, forecasts: Optional[Tuple] = None):
        self.L = _lib.lib()
        _need_gpu()
        self.device = dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.n_slots, self.seg_len, self.ring_len, self.num_transform = int(n_slots), int(seg_len), int(ring_len), int(num_transform)
        self.vid_res = _vid_res(vid_res, "two finite numbers")
        self._stats = _scaler_stats(center, scale, dev)
        with torch.cuda.device(dev):
            self.ring = torch.zeros(self.n_slots * 2 * self.ring_len * 34, device=dev, dtype=torch.float32)
            self.frame_scores_ring = torch.zeros(self.n_slots, self.num_transform, self.ring_len, device=dev, dtype=torch.float32)
        self._state = _lib.StreamState(ring=self.ring.data_ptr(), frame_scores=self.frame_scores_ring.data_ptr(),
                                       n_slots=self.n_slots, ring_len=self.ring_len, seg_len=self.seg_len,
                                       num_transform=self.num_transform)
        # joint_scores: the per-joint ring (mcd_stream_joint_state_t) beside the two above; without it nothing is allocated
        self.joint_scores_ring, self._jstate = None, None
        if joint_scores:
            with torch.cuda.device(dev):
                self.joint_scores_ring = torch.zeros(self.n_slots, self.num_transform, self.ring_len, 17, device=dev, dtype=torch.float32)
            self._jstate = _lib.StreamJointState(joint_scores=self.joint_scores_ring.data_ptr())
        # forecasts = (method, spread, n_corrupt): the forecast and observed rings (mcd_stream_forecast_state_t); without it nothing
        # is allocated.  (method, spread, n_corrupt, 'all'): the forecast ring of EVERY transform instead, (n_slots, ring_len,
        # num_transform, n_corrupt, 34), and the inverse table of the transforms (mcd_stream_forecast_tta_state_t); the ring of
        # transform 0 alone is not allocated then, nor this one under 'identity'
        self.forecast_ring, self.observed_ring, self._fstate, self._forecast = None, None, None, None
        self.forecast_tta_ring, self.inv_affine, self._tstate = None, None, None
        if forecasts is not None:
            method, spread, n_corrupt = forecasts[:3]
            transforms = forecasts[3] if len(forecasts) > 3 else "identity"
            self._forecast = forecast_codes(method, spread, ("forecast method", "forecast spread"))
            if not 1 <= int(n_corrupt) <= _lib.MCD_MAX_FRAMES:
                raise ValueError(f"n_corrupt must be in 1 .. {_lib.MCD_MAX_FRAMES}, got {n_corrupt}")
            if transforms not in ("identity", "all"):
                raise ValueError(f"forecast transforms must be 'identity' or 'all', got {transforms!r}")
            if transforms == "all" and self.num_transform * int(n_corrupt) > _lib.MCD_FORECAST_VIEW_COVER:
                raise ValueError(f"forecast transforms 'all': num_transform * n_corrupt = {self.num_transform} * {int(n_corrupt)} exceeds "
                                 f"{_lib.MCD_FORECAST_VIEW_COVER}, the forecasts one row's reduction holds")
            with torch.cuda.device(dev):      # (zeros: the kernels need no initial value, two streams in one state compare equal)
                self.observed_ring = torch.zeros(self.n_slots, self.ring_len, 34, device=dev, dtype=torch.float32)
                if transforms == "all":
                    from .utils.transforms import inverse_affine_table
                    self.forecast_tta_ring = torch.zeros(self.n_slots, self.ring_len, self.num_transform, int(n_corrupt), 34, device=dev,
                                                         dtype=torch.float32)
                    self.inv_affine = inverse_affine_table(self.num_transform).to(dev)
                    self._tstate = _lib.StreamForecastTtaState(forecast=self.forecast_tta_ring.data_ptr(), observed=self.observed_ring.data_ptr(),
                                                               n_corrupt=int(n_corrupt), num_transform=self.num_transform)
                else:
                    self.forecast_ring = torch.zeros(self.n_slots, self.ring_len, int(n_corrupt), 34, device=dev, dtype=torch.float32)
                    self._fstate = _lib.StreamForecastState(forecast=self.forecast_ring.data_ptr(), observed=self.observed_ring.data_ptr(),
                                                            n_corrupt=int(n_corrupt))

    def _forecast_outputs(self, rows: int):
        dev = self.device
        return (torch.empty(rows, 34, device=dev, dtype=torch.float32), torch.empty(rows, 34, device=dev, dtype=torch.float32),
                torch.empty(rows, 34, device=dev, dtype=torch.float32), torch.empty(rows, device=dev, dtype=torch.int32),
                torch.empty(rows, device=dev, dtype=torch.float32))

    def forecast_group(self, raw: torch.Tensor, desc: torch.Tensor, n: int, loss_all: Optional[torch.Tensor],
                       poses_all: Optional[torch.Tensor], win: Optional[torch.Tensor], n_windows: int, cfg: "_lib.ScoreCfg",
                       aggregation: str):
        """mcd_stream_forecast_group, behind the group's scoring call: raw / desc as for push_group, loss_all (num_transform *
        n_windows, S) and poses_all (num_transform * n_windows, S, 2, Tx, 17) of that call, win as for frame_scores_group, cfg: the
        model's frame lists and sample count, aggregation 'best' | 'worst' -> (expected (n_windows, 34) pixels, expected_norm
        (n_windows, 34), observed (n_windows, 34), count (n_windows,) int32, spread (n_windows,)) in (tick, j) order: the row each
        window finalised.  A group without a window (n_windows = 0) only stores its raw rows."""
        nw = int(n_windows)
        with torch.cuda.device(self.device):
            out = self._forecast_outputs(nw)
            c, s = self._stats
            if self._tstate is not None:      # every transform: mcd_stream_forecast_group_tta, the same call plus the inverse table
                _lib.check(self.L.mcd_stream_forecast_group_tta(
                    C.byref(self._state), C.byref(self._tstate), _ptr(raw), _ptr(desc), int(n), _ptr(loss_all) if nw else None,
                    _ptr(poses_all) if nw else None, _ptr(win) if nw else None, nw, C.byref(cfg), _lib.AGGR[aggregation], self._forecast[0],
                    self._forecast[1], self.vid_res[0], self.vid_res[1], _ptr(c), _ptr(s), _ptr(self.inv_affine),
                    *(_ptr(o) if nw else None for o in out), _stream()))
                return out
            _lib.check(self.L.mcd_stream_forecast_group(
                C.byref(self._state), C.byref(self._fstate), _ptr(raw), _ptr(desc), int(n), _ptr(loss_all) if nw else None,
                _ptr(poses_all) if nw else None, _ptr(win) if nw else None, nw, C.byref(cfg), _lib.AGGR[aggregation], self._forecast[0],
                self._forecast[1], self.vid_res[0], self.vid_res[1], _ptr(c), _ptr(s), *(_ptr(o) if nw else None for o in out), _stream()))
        return out

    def forecast_flush(self, win: Optional[torch.Tensor], n: int, cfg: "_lib.ScoreCfg"):
        """mcd_stream_forecast_flush: as `flush` -> the five tensors of forecast_group with n * (seg_len - 1) rows."""
        with torch.cuda.device(self.device):
            out = self._forecast_outputs(int(n) * (self.seg_len - 1))
            if out[3].numel() and self._tstate is not None:
                c, s = self._stats
                _lib.check(self.L.mcd_stream_forecast_flush_tta(
                    C.byref(self._state), C.byref(self._tstate), _ptr(win), int(n), C.byref(cfg), self._forecast[0], self._forecast[1],
                    self.vid_res[0], self.vid_res[1], _ptr(c), _ptr(s), _ptr(self.inv_affine), *(_ptr(o) for o in out), _stream()))
            elif out[3].numel():
                c, s = self._stats
                _lib.check(self.L.mcd_stream_forecast_flush(
                    C.byref(self._state), C.byref(self._fstate), _ptr(win), int(n), C.byref(cfg), self._forecast[0], self._forecast[1],
                    self.vid_res[0], self.vid_res[1], _ptr(c), _ptr(s), *(_ptr(o) for o in out), _stream()))
        return out

    def joint_scores_group(self, maps: torch.Tensor, win: torch.Tensor, n_windows: int, cfg: "_lib.ScoreCfg") -> torch.Tensor:
        """mcd_stream_joint_scores_group: maps (num_transform * n_windows, Tx, 17) error maps of the group's windows in the order
        of push_group's base, win as for frame_scores_group, cfg: the model's frame lists -> (n_windows, num_transform, 17) final
        per-joint frame scores in (tick, j) order."""
        with torch.cuda.device(self.device):
            final = torch.empty(int(n_windows), self.num_transform, 17, device=self.device, dtype=torch.float32)
            _lib.check(self.L.mcd_stream_joint_scores_group(C.byref(self._state), C.byref(self._jstate), _ptr(maps), _ptr(win),
                                                            int(n_windows), C.byref(cfg), _ptr(final), _stream()))
        return final

    def joint_flush(self, win: Optional[torch.Tensor], n: int) -> torch.Tensor:
        """mcd_stream_joint_flush: as `flush` -> (n * (seg_len - 1), num_transform, 17)."""
        with torch.cuda.device(self.device):
            out = torch.empty(int(n) * (self.seg_len - 1), self.num_transform, 17, device=self.device, dtype=torch.float32)
            if out.numel():
                _lib.check(self.L.mcd_stream_joint_flush(C.byref(self._state), C.byref(self._jstate), _ptr(win), int(n), _ptr(out),
                                                         _stream()))
        return out

    def push_group(self, raw: torch.Tensor, desc: torch.Tensor, n: int, n_windows: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """mcd_stream_push_group: the rows of a group of ticks, raw (n, 34) fp32, desc (n, 4) int32 [slot, row index, batch
        position of the row's window under transform 0 | -1, windows of its tick] (device; any dtype of 4 bytes: views of one
        staging buffer) -> (base (num_transform * n_windows,) int64, trans (same,) int32), tick-major, inside a tick
        transform-major."""
        nw = self.num_transform * int(n_windows)
        with torch.cuda.device(self.device):
            base = torch.empty(nw, device=self.device, dtype=torch.int64)
            trans = torch.empty(nw, device=self.device, dtype=torch.int32)
            c, s = self._stats
            _lib.check(self.L.mcd_stream_push_group(C.byref(self._state), _ptr(raw), _ptr(desc), int(n), int(n_windows),
                                                    self.vid_res[0], self.vid_res[1], _ptr(c), _ptr(s), _ptr(base), _ptr(trans),
                                                    _stream()))
        return base, trans

    def frame_scores_group(self, scores: torch.Tensor, win: torch.Tensor, n_windows: int) -> torch.Tensor:
        """mcd_stream_frame_scores_group: scores (num_transform * n_windows,) fp32 in the order of push_group's base, win
        (n_windows, 5) int32 [slot, r_last, batch position under transform 0, windows of its tick, index in (tick, j) order]
        sorted by slot, then row -> (n_windows, num_transform) final frame scores in (tick, j) order."""
        with torch.cuda.device(self.device):
            final = torch.empty(int(n_windows), self.num_transform, device=self.device, dtype=torch.float32)
            _lib.check(self.L.mcd_stream_frame_scores_group(C.byref(self._state), _ptr(scores), _ptr(win), int(n_windows),
                                                            _ptr(final), _stream()))
        return final

    def flush(self, win: Optional[torch.Tensor], n: int) -> torch.Tensor:
        """mcd_stream_flush: win (n, 2) int32 [slot, last row index] of tracks being closed -> (n * (seg_len - 1), num_transform)
        frame scores of their pending rows, oldest first."""
        with torch.cuda.device(self.device):
            out = torch.empty(int(n) * (self.seg_len - 1), self.num_transform, device=self.device, dtype=torch.float32)
            if out.numel():
                _lib.check(self.L.mcd_stream_flush(C.byref(self._state), _ptr(win), int(n), _ptr(out), _stream()))
        return out


class ClipRings:
    """Device state of the online clip scores of a live pose stream (mcd_clip_state_t) and the two launches on it; the host half
    -- which frame of which clip sits in which cell, what is complete, what was emitted -- is mocodad_amd.stream.ClipTable.
      sum, lmax, lmin  (n_clips, num_transform, clip_ring_len) fp64: the person aggregate of one video frame per cell
      n                (same) int32: persons added
      gauss            (2 radius + 1,) fp64: utils/eval_utils.gaussian_kernel1d(sigma)
    All calls are asynchronous on the current stream; one state is driven from one stream."""

    def __init__(self, n_clips: int, clip_ring_len: int, num_transform: int, sigma: float, shift: int, *, device=None):
        from .utils.eval_utils import gaussian_kernel1d
        self.L = _lib.lib()
        _need_gpu()
        self.device = dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.n_clips, self.clip_ring_len, self.num_transform = int(n_clips), int(clip_ring_len), int(num_transform)
        w = gaussian_kernel1d(sigma)
        self.radius, self.shift = (len(w) - 1) // 2, int(shift)
        shape = (self.n_clips, self.num_transform, self.clip_ring_len)
        with torch.cuda.device(dev):
            self.sum, self.lmax, self.lmin = (torch.zeros(shape, device=dev, dtype=torch.float64) for _ in range(3))
            self.n = torch.zeros(shape, device=dev, dtype=torch.int32)
            self.gauss = torch.from_numpy(w).to(dev)
        self._state = _lib.ClipState(sum=self.sum.data_ptr(), lmax=self.lmax.data_ptr(), lmin=self.lmin.data_ptr(),
                                     n=self.n.data_ptr(), n_clips=self.n_clips, clip_ring_len=self.clip_ring_len,
                                     num_transform=self.num_transform)

    def update(self, runs: torch.Tensor, n_runs: int, contrib: Optional[torch.Tensor], n_contrib: int,
               finals: Optional[torch.Tensor], tails: Optional[torch.Tensor]) -> None:
        """mcd_stream_clip_update: runs (n_runs, 5) int32 [clip slot, ring position, first contribution, count, zero-first],
        contrib (n_contrib, 2) int32 [0 = finals | 1 = tails, row]; finals / tails (rows, num_transform) fp32 or None."""
        nf = int(finals.shape[0]) if finals is not None and finals.numel() else 0
        ntl = int(tails.shape[0]) if tails is not None and tails.numel() else 0
        with torch.cuda.device(self.device):
            _lib.check(self.L.mcd_stream_clip_update(C.byref(self._state), _ptr(runs), int(n_runs), _ptr(contrib) if n_contrib else None,
                                                     int(n_contrib), _ptr(finals) if nf else None, nf, _ptr(tails) if ntl else None,
                                                     ntl, _stream()))

    def emit(self, outs: Optional[torch.Tensor], n_out: int) -> torch.Tensor:
        """mcd_stream_clip_emit: outs (n_out, 4) int32 [clip slot, frame offset from the origin, segment length | -1, ring position
        of the origin] -> (n_out,) fp64 clip scores."""
        with torch.cuda.device(self.device):
            out = torch.empty(int(n_out), device=self.device, dtype=torch.float64)
            if n_out:
                _lib.check(self.L.mcd_stream_clip_emit(C.byref(self._state), _ptr(outs), int(n_out), _ptr(self.gauss), self.radius,
                                                       self.shift, _ptr(out), _stream()))
        return out


class FrameScoreAssembler:
    """Window scores -> per-frame anomaly scores on the device (mcd_frame_scores): the whole of the reference's
    post_processing loops (mocodad.py:362-425) except roc_auc_score.  Built once per dataset from the ground-truth masks."""

    MAX_WORKSPACE = 8 << 30

    def __init__(self, gts, masks, *, num_transform: int, pad_size: int, filter_kernel_size: float, frames_shift: int, device):
        from .utils.eval_utils import frame_tables, gaussian_kernel1d
        self.L = _lib.lib()
        self.device = torch.device(device)
        t = frame_tables(gts, masks)
        self.gt, self.total, self.F = t["gt"], int(t["total"]), int(t["max_frames"])
        w = gaussian_kernel1d(filter_kernel_size)
        self._dev = {k: torch.from_numpy(np.ascontiguousarray(t[k])).to(self.device)
                     for k in ("clip_keys", "clip_n_frames", "frame_dst", "clip_out_len", "clip_out_off")}
        self._dev["gauss"] = torch.from_numpy(w).to(self.device)
        self.n_clips, self.num_transform = len(t["clip_keys"]), int(num_transform)
        self.pad_size, self.frames_shift, self.radius = int(pad_size), int(frames_shift), (len(w) - 1) // 2
        self._ws = None

    def _cfg(self, n_persons: int) -> "_lib.FrameCfg":
        d = self._dev
        return _lib.FrameCfg(n_clips=self.n_clips, num_transform=self.num_transform, n_persons=n_persons, max_frames=self.F,
                             pad_size=self.pad_size, frames_shift=self.frames_shift, gauss_radius=self.radius,
                             clip_keys=d["clip_keys"].data_ptr(), clip_n_frames=d["clip_n_frames"].data_ptr(),
                             frame_dst=d["frame_dst"].data_ptr(), clip_out_len=d["clip_out_len"].data_ptr(),
                             clip_out_off=d["clip_out_off"].data_ptr(), gauss_weights=d["gauss"].data_ptr())

    def __call__(self, scores, trans, meta, frames) -> Optional[np.ndarray]:
        """scores (N,), trans (N,), meta (N,4), frames (N,seg_len): arrays or tensors, host or device -> pds (total,) float64
        (None if the dense (transform, clip, person) table would not fit the workspace cap: the caller falls back to the host)."""
        dev = self.device
        # Host arrays (what processing_data hands over) are checked on the host: the same checks as torch device ops cost a lazy
        # code-object load per op on first use (isfinite, >=, &, all, max: ~80 ms of a cold epoch end, tools/postproc_time.py)
        ok = npers = None
        if not torch.is_tensor(scores) and not torch.is_tensor(meta):
            sc_h, me_h = np.asarray(scores), np.asarray(meta)
            if sc_h.size:
                ok = bool((np.isfinite(sc_h) & (sc_h >= 0)).all())
                npers = int(me_h[:, 2].max()) + 1 if me_h.ndim == 2 and me_h.shape[1] == 4 else None
        as_t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, dt).contiguous()
        scores, trans, meta, frames = as_t(scores, torch.float32), as_t(trans, torch.int64), as_t(meta, torch.int64), as_t(frames, torch.int32)
        n = int(scores.numel())
        if meta.shape != (n, 4) or trans.numel() != n or frames.shape[0] != n:
            raise ValueError("scores / trans / meta / frames disagree on the number of windows")
        # the scatter-max orders non-negative floats by their bit patterns: a NaN / negative / infinite window score (a
        # diverged model) must surface as an error here, not as a plausible-looking AUC (the reference's NumPy path lets the
        # NaN reach roc_auc_score, which raises)
        if ok is None:
            ok = (not n) or bool((torch.isfinite(scores) & (scores >= 0)).all().item())
        if not ok:
            raise ValueError("window scores must be finite and non-negative (got NaN / inf / negative values: diverged model?)")
        n_persons = (npers if npers is not None else int(meta[:, 2].max().item()) + 1) if n else 1
        cfg = self._cfg(max(n_persons, 1))
        need = int(self.L.mcd_frame_scores_workspace_bytes(C.byref(cfg)))
        if need > self.MAX_WORKSPACE:
            return None
        with torch.cuda.device(dev):
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, device=dev, dtype=torch.uint8)
            out = torch.empty(self.total, device=dev, dtype=torch.float64)
            _lib.check(self.L.mcd_frame_scores(C.byref(cfg), _ptr(scores), _ptr(trans), _ptr(meta), _ptr(frames), n,
                                               int(frames.shape[1]) if n else 1, _ptr(self._ws), _ptr(out), _stream()))
        pds = out.cpu().numpy()
        if np.isnan(pds).any():
            raise ValueError("a (transform, clip) block has no pose windows (need at least one array to stack)")
        return pds
