"""Drop-in for the reference's models/mocodad_latent.py::MoCoDADlatent (stage 'diffusion') on MI355X.

Same constructor keys (`stage`, `latent_embedding_dim`, `hidden_sizes`, `pretrained_model_ckpt_path` on top of MoCoDAD's), the
same state_dict key layout (a diffusion-stage Lightning checkpoint holds every entry, so `pretrained_model_ckpt_path` is not read
at evaluation) and the same `forward` lists -- but the encoder (condition encoder + the U-Net's down path + to_time_dim) and the
reverse-diffusion chain over the latent (the conditioned MLP denoiser, the DDPM updates, the loss, the loss-based aggregation)
run in the HIP launches behind mcd_latent_score (mocodad_amd.engine.LatentScorer): two for the shipped configuration, three
(the condition encoder as its own launch) for `E_unet` or another number of condition frames, four (a gather of the condition
frames in front) for another channel list / h_dim.
3 or 5 .. 12 corrupt frames (e.g. seg_len 12 or 24 split in halves); at 5 .. 12 the condition encoder is always its own launch and
to_time_dim is one more launch between the encoder and the chain.

Reference: models/mocodad_latent.py (forward :69-132), models/common/components.py:203-291 (Denoiser),
models/stsae/stsae_unet.py:8-251 (STSE_Unet).  `stage: pretrain` is mocodad_latent_pretrain.MoCoDADlatentPretrain; training is outside
the accelerated path.

Extension, pose space: the reference trains the diffusion stage with `model` and `condition_encoder` loaded from the stage-1
checkpoint and frozen (mocodad_latent.py:223-228), so stage 1's rev_to_time_dim and up path decode the latents this stage
generates.  `load_decoder` takes them from the stage-1 checkpoint (`pretrained_model_ckpt_path`); `latent_score_space: 'pose'`
(or forward(space='pose')) then decodes the S generated latents of every window (mcd_latent_decode_samples), takes the loss against
the window's corrupt frames and aggregates as the pose model does -- which is what `return_maps` and the *_pose aggregations need.
"""
import argparse
import os
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import mocodad as _pose
from .mocodad import JointResampleParams, MoCoDAD, _stack


class LatentUNetParams(nn.Module):
    """Parameter tree of STSE_Unet as MoCoDADlatent builds it (mocodad_latent.py:51-55): the U-Net's down path WITH the layers'
    embedding Linears, ending in 64 channels, + to_time_dim onto the latent."""
    down_channels = [16, 32, 32, 64, 64, 128, 64]

    def __init__(self, c_in: int, embedding_dim: int, latent_dim: int, n_frames: int, dropout: float):
        super().__init__()
        d, T, e = self.down_channels, n_frames, embedding_dim
        self.st_gcnnsp1a = _stack([(c_in, d[0])], T, 17, dropout, e)
        self.st_gcnnsd1 = _stack([(d[0], d[1]), (d[1], d[2])], T, 17, dropout, e)
        self.st_gcnnsd2 = _stack([(d[2], d[3]), (d[3], d[4])], T, 12, dropout, e)
        self.st_gcnnsd3 = _stack([(d[4], d[5]), (d[5], d[6])], T, 10, dropout, e)
        self.down1 = JointResampleParams(17, 12, dropout)
        self.down2 = JointResampleParams(12, 10, dropout)
        self.to_time_dim = nn.Linear(d[6] * T * 10, latent_dim)


class DenoiserParams(nn.Module):
    """Parameter tree of Denoiser (components.py:228-241): Linear -> BatchNorm1d -> ReLU per hidden size, the last a plain Linear
    whose input is the previous hidden size; one cond_layers Linear per layer."""

    def __init__(self, input_size: int, hidden_sizes: List[int], cond_size: int):
        super().__init__()
        self.net = nn.ModuleList()
        self.cond_layers = nn.ModuleList()
        n = len(hidden_sizes)
        for idx, nxt in enumerate(hidden_sizes):
            self.cond_layers.append(nn.Linear(cond_size, nxt))
            if idx == n - 1:
                self.net.append(nn.Linear(input_size, nxt))
            else:
                self.net.append(nn.Sequential(nn.Linear(input_size, nxt), nn.BatchNorm1d(nxt), nn.ReLU(inplace=True)))
                input_size = nxt


LOSS_FNS = {"smooth_l1": F.smooth_l1_loss, "l1": F.l1_loss, "mse": F.mse_loss}
SCORE_SPACES = ("latent", "pose")
# the tensors the two stages' checkpoints share (frozen while stage 2 trains): everything of this module's `model` -- the down path
# and to_time_dim -- and the condition encoder
SHARED_PREFIXES = ("model.", "condition_encoder.")


class LatentStage(MoCoDAD):
    """What the two stages of the latent model share (MoCoDADlatent here, mocodad_latent_pretrain.MoCoDADlatentPretrain): the
    constructor keys on top of MoCoDAD's, 'inject' as the only conditioning, and the arguments of their engine handle.  A stage
    checks `args.stage` and sets `hidden_sizes` before it calls this constructor."""
    is_latent = True

    def __init__(self, args: argparse.Namespace) -> None:
        self.stage = args.stage
        self.latent_embedding_dim = args.latent_embedding_dim
        self.pretrained_model_ckpt_path = getattr(args, "pretrained_model_ckpt_path", None)
        super().__init__(args)
        assert self.conditioning_strategy == 'inject', 'Conditioning strategy must be inject. Other strategies are not supported for the latent space'

    def _scorer_kwargs(self, device) -> dict:
        """The keyword arguments engine.LatentScorer and engine.LatentReconstructor share, from this module."""
        if self.conditioning_strategy != "inject":
            raise NotImplementedError("the latent model conditions by 'inject' only")
        ci, xi = self._frame_split()
        # (the class as the pose module holds it NOW: build_model, inherited, takes it from that module's globals, and a reload
        # of mocodad_amd.models.mocodad rebinds it there -- a name imported into this module would be the class of before)
        unet = isinstance(self.condition_encoder, _pose.CondUNetParams)
        return dict(seg_len=self.n_frames, cond_idx=ci, corrupt_idx=xi, cond_unet=unet,
                    cond_channels=[] if unet else list(self.condition_encoder.channels), latent_dim=self.latent_embedding_dim,
                    num_coords=self.num_coords, n_joints=self.n_joints, emb_dim=self.embedding_dim, device=device)


class MoCoDADlatent(LatentStage):
    def __init__(self, args: argparse.Namespace) -> None:
        self.hidden_sizes = list(args.hidden_sizes)
        if args.stage == "pretrain":
            raise NotImplementedError("MoCoDADlatent (mocodad_amd) is the 'diffusion' stage; a stage-1 checkpoint is evaluated by "
                                      "mocodad_amd.models.mocodad_latent_pretrain.MoCoDADlatentPretrain (training: the reference implementation)")
        if args.stage != "diffusion":
            raise ValueError(f"Unknown stage {args.stage}")
        self.latent_score_space = self._check_space(getattr(args, "latent_score_space", None) or "latent")
        super().__init__(args)
        self._decoder_sd = None       # load_decoder: the autoencoder's state_dict (a plain dict: no parameter of this module)
        self._decoder = None          # ... its engine.LatentReconstructor, built lazily per device
        self._decoder_key = None
        self._pose_scorer = None      # engine.LatentPoseScorer over the two, rebuilt when either is

    @staticmethod
    def _check_space(space: str) -> str:
        if space not in SCORE_SPACES:
            raise ValueError(f"latent_score_space must be one of {SCORE_SPACES}, got {space!r}")
        return space

    def build_model(self) -> None:
        super().build_model()
        self.model = LatentUNetParams(self.num_coords, self.embedding_dim, self.latent_embedding_dim, self.n_frames_corrupt, self.dropout)
        self.denoiser = DenoiserParams(self.latent_embedding_dim, self.hidden_sizes, self.embedding_dim)
        self.eval()

    def build_scorer(self, device):
        """engine.LatentScorer with this module's weights (MoCoDAD.scorer() caches it per device)."""
        from ..engine import LatentScorer
        return LatentScorer(self.state_dict(), hidden_sizes=self.hidden_sizes, **self._scorer_kwargs(device))

    # -------------------------------------------------------------- the stage-1 decoder
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        self._decoder_sd = self._decoder = self._pose_scorer = None      # (its copies of the shared tensors are stale: call load_decoder again)
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def load_decoder(self, source=None, *, check: bool = True) -> None:
        """Takes the decoder of the generated latents -- rev_to_time_dim and the up path -- from a stage-1 ('pretrain') checkpoint.
        source: its state_dict, a checkpoint path, or None = `pretrained_model_ckpt_path`.  The autoencoder handle is packed from
        the stage-1 tensors this module lacks plus this module's OWN down path, to_time_dim and condition encoder.
        check: every tensor the two stages share must be torch.equal between the checkpoint and this module (they are when stage 2
        was trained from that checkpoint with both frozen); ValueError naming the first key that is not.  check=False skips that.
        Nothing is registered: state_dict() and loading a diffusion checkpoint are what they were (load_state_dict drops the
        decoder: call this after it)."""
        if source is None:
            source = self.pretrained_model_ckpt_path
            if not source:
                raise ValueError("load_decoder: no source given and pretrained_model_ckpt_path is not set")
        if isinstance(source, (str, os.PathLike)):
            if not os.path.exists(source):
                raise FileNotFoundError(f"load_decoder: stage-1 checkpoint {source} not found")
            source = torch.load(source, map_location="cpu", weights_only=False)
            source = source.get("state_dict", source)
        own = self.state_dict()
        shared = [k for k in own if k.startswith(SHARED_PREFIXES)]
        if check:
            for k in shared:
                if k not in source:
                    raise ValueError(f"load_decoder: the stage-1 checkpoint has no tensor {k!r}")
                a, b = source[k].detach().cpu(), own[k].detach().cpu()
                if a.shape != b.shape or not torch.equal(a, b):
                    raise ValueError(f"load_decoder: tensor {k!r} differs between the stage-1 checkpoint and this module "
                                     "(the stages share the down path, to_time_dim and the condition encoder; check=False decodes "
                                     "with this module's own)")
        for k in ("model.rev_to_time_dim.weight", "model.rev_to_time_dim.bias"):
            if k not in source:
                raise ValueError(f"load_decoder: the stage-1 checkpoint has no tensor {k!r} (not a 'pretrain' checkpoint?)")
        # the decoder half of stage 1 (what `model` holds there and not here: the up path, rev_to_time_dim) + this module's own tensors
        sd = {k: v.detach().clone().cpu() for k, v in source.items() if torch.is_tensor(v) and k.startswith("model.") and k not in own}
        sd.update({k: own[k].detach().clone().cpu() for k in shared})
        self._decoder_sd, self._decoder, self._decoder_key, self._pose_scorer = sd, None, None, None

    def decoder(self):
        """engine.LatentReconstructor of the loaded decoder on the module's current device (packed lazily, like scorer())."""
        if self._decoder_sd is None:
            raise RuntimeError("MoCoDADlatent has no decoder: call load_decoder(stage-1 state_dict or checkpoint path) first")
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} (mocodad_amd) scores on an MI355X only: move the module to a cuda device "
                               "(there is no CPU fallback)")
        if self._decoder is None or self._decoder_key != str(dev):
            from ..engine import LatentReconstructor
            self._decoder = LatentReconstructor(self._decoder_sd, **self._scorer_kwargs(dev))
            self._decoder_key = str(dev)
        return self._decoder

    def pose_scorer(self):
        """engine.LatentPoseScorer over scorer() and decoder(): pose-space scoring as one library call (built lazily, like both)."""
        sc, dec = self.scorer(), self.decoder()
        ps = self._pose_scorer
        if ps is None or ps.scorer is not sc or ps.decoder is not dec:
            from ..engine import LatentPoseScorer
            ps = self._pose_scorer = LatentPoseScorer(sc, dec)
        return ps

    # -------------------------------------------------------------- forward
    def _loss(self, x: torch.Tensor, z0: torch.Tensor) -> torch.Tensor:
        return LOSS_FNS[self.loss_name](x, z0.expand_as(x), reduction="none").mean(dim=-1)

    def forward(self, input_data: List[torch.Tensor], condition_data: torch.Tensor = None, aggr_strategy: str = 'best', *,
                return_: str = None, noise: Optional[torch.Tensor] = None, window_offset: Optional[int] = None,
                return_maps: bool = False, space: Optional[str] = None, return_samples: bool = False) -> List[torch.Tensor]:
        """[data (B,C,T,V), transformation_idx, metadata, actual_frames] -> [loss and/or selected latent] + the inputs, as
        mocodad_latent.py:69-129 (`condition_data` is unused there too; `aggr_strategy` defaults to 'best', None = the module's).

        noise (extension, keyword only): (S, max(ns-1,1), B, D) replacing the in-kernel Philox stream -- slot 0 = the x_T of
        torch.randn (:109), slot k = the randn_like of step ns-k (:121), in call order.  window_offset keys the Philox stream.
        space (extension, keyword only; None = the module's `latent_score_space`): 'latent' -- the list above, the loss taken on
        the latent -- or 'pose' (needs load_decoder): the S generated latents of every window are decoded to forecasts, the loss
        is taken against the window's corrupt frames and aggregated as MoCoDAD.forward does, every strategy of the pose model
        included (mean_pose / median_pose on poses); return_ 'pose' gives the selected decoded forecast (B,2,Tx,17).
        return_maps: with a decoder it implies pose space and appends maps (B,Tx,V) and map_frames (B,Tx) exactly as
        MoCoDAD.forward does (mcd_error_maps on the decoded forecasts).  Without one: NotImplementedError -- the error maps are
        per joint and forecast frame, and a latent has no joints.
        return_samples (pose space only; off: exactly the list above): appends poses_all (B,S,2,Tx,V), every decoded sample of every
        window (what aggr_strategy 'all' returns as its pose), and map_frames (B,Tx), behind the entries of return_maps; the call
        runs as the sequence of engine calls, whose losses the one-call path reproduces bit for bit."""
        if return_maps and self._decoder_sd is None:
            raise NotImplementedError("MoCoDADlatent has no error maps: its loss is taken on a latent code, and a latent has no joints "
                                      "(return_maps is for the pose model, MoCoDAD -- or call load_decoder first: the stage-1 "
                                      "decoder turns the generated latents into forecasts)")
        space = "pose" if return_maps else self._check_space(self.latent_score_space if space is None else space)
        if space == "pose":
            if self._decoder_sd is None:
                raise RuntimeError("latent_score_space 'pose' needs the stage-1 decoder: call load_decoder first")
            return self._forward_pose(input_data, aggr_strategy, return_, noise, window_offset, return_maps, return_samples)
        if return_samples:
            raise ValueError("return_samples: in latent space the model generates latent codes, not poses (space='pose' decodes them)")
        tensor_data, meta_out, aggr, ret, sc, _, kw = self._begin_forward(input_data, aggr_strategy, return_, noise, window_offset)
        loss_based = aggr in ("mean", "median") or "quantile" in aggr
        if (loss_based or aggr in ("best", "worst")) and (ret == "loss" or loss_based):
            loss, _, _, _ = sc.score(tensor_data, aggregation=aggr, **kw)         # both launches; one loss per window comes back
            selected = None
        else:
            _, loss_all, lat, z0 = sc.score(tensor_data, aggregation="all", want_latents=True, want_code=True, **kw)
            selected, loss = self._aggregate_latents(lat, loss_all, z0, aggr)
        return self._pack_out_data(selected, loss, [tensor_data] + meta_out, return_=ret)

    def _forward_pose(self, input_data, aggr_strategy, return_, noise, window_offset, return_maps, return_samples=False) -> List[torch.Tensor]:
        """forward in pose space: the chain call for the latents and cond_emb, the decoder on all samples, then the pose model's
        aggregation (and error maps) on (loss_all, pose_all) -- for the loss-based aggregations as ONE library call (pose_scorer()),
        for mean_pose / median_pose / all / random as the sequence of engine calls."""
        for kw_name, on in (("return_maps", return_maps), ("return_samples", return_samples)):
            if on and (self.aggregation_strategy if aggr_strategy is None else aggr_strategy) == "random":
                raise ValueError(f"{kw_name}: the 'random' aggregation keeps no record of the sample it drew; use 'all' and index it")
        tensor_data, meta_out, aggr, ret, sc, _, kw = self._begin_forward(input_data, aggr_strategy, return_, noise, window_offset)
        dec = self.decoder()
        if not return_samples and (aggr in ("best", "worst", "mean", "median") or "quantile" in aggr):
            # the loss-based aggregations: ONE library call (mcd_latent_score_pose), the bits of the sequence below
            r = self.pose_scorer().score(tensor_data, aggregation=aggr, want_maps=return_maps, want_selected=ret in ("pose", "all"), **kw)
            out = self._pack_out_data(r[4] if len(r) > 4 else None, r[0], [tensor_data] + meta_out, return_=ret)
            return out + [r[3], self.map_frames(None, r[3].shape[0])] if return_maps else out
        want_pose = ret in ("pose", "all") or aggr in ("all", "random", "mean_pose", "median_pose")
        if hasattr(tensor_data, "as_view") and aggr in ("mean_pose", "median_pose"):
            tensor_data = tensor_data.materialize()      # the *_pose strategies compare against the windows themselves
        _, _, lat, _, cond = sc.score(tensor_data, aggregation="all", want_latents=True, want_cond=True, **kw)
        poses_all, loss_all = dec.decode_samples(tensor_data, lat, cond, want_poses=want_pose or return_maps or return_samples,
                                                 loss_fn=self.loss_name)
        selected, loss = self._aggregate(dec, tensor_data, loss_all, poses_all, aggr, want_pose)
        out = self._pack_out_data(selected, loss, [tensor_data] + meta_out, return_=ret)
        if return_maps:
            maps = dec.error_maps(tensor_data, loss_all, poses_all, aggr, loss_fn=self.loss_name)
            out = out + [maps, self.map_frames(None, maps.shape[0])]
        return out + [poses_all, self.map_frames(None, poses_all.shape[0])] if return_samples else out

    def _aggregate_latents(self, lat: torch.Tensor, loss_all: torch.Tensor, z0: torch.Tensor, aggr: str):
        """_aggregation_strategy (mocodad.py:454-520) on the (B,S,D) latents and (B,S) losses the chain launch wrote: device
        tensor ops, not the hot path."""
        if aggr == "all":
            return lat, loss_all
        if aggr == "random":      # (the reference returns a bare tensor here, mocodad.py:480-481; like the parent: the sample and its loss)
            s = int(np.random.randint(loss_all.shape[1]))
            return lat[:, s], loss_all[:, s]
        if aggr == "mean_pose":
            sel = lat.mean(dim=1)
            return sel, self._loss(sel, z0)
        if aggr == "median_pose":
            sel = torch.median(lat, dim=1).values
            return sel, self._loss(sel, z0)
        if aggr in ("best", "worst"):
            best = aggr == "best"
            loss = torch.full((lat.shape[0],), 1e10 if best else -1.0, device=lat.device)
            sel = torch.zeros_like(z0)
            for s in range(lat.shape[1]):
                m = loss_all[:, s] < loss if best else loss_all[:, s] > loss
                loss = torch.where(m, loss_all[:, s], loss)
                sel = torch.where(m[:, None], lat[:, s], sel)
            return sel, loss
        raise ValueError(f"Unknown aggregation strategy {aggr}")
