"""Drop-in for the reference's models/mocodad_latent.py::MoCoDADlatent at stage 'pretrain' on MI355X: the bottleneck autoencoder
a stage-1 checkpoint holds -- STSAE_Unet(use_bottleneck=True, inject_condition=True) (mocodad_latent.py:58-64) and the condition
encoder -- evaluated the way the reference selects such a checkpoint: one pass at the constant time step -1 returns the
reconstructed corrupt frames, and post_processing is the mean loss_fn(reconstruction, corrupt frames) (`pretrain_rec_loss`,
mocodad_latent.py:130-132, 192-220).

Same constructor keys as MoCoDADlatent (`stage` must be 'pretrain'; the diffusion stage is mocodad_latent.MoCoDADlatent) and the
same state_dict key layout.  The pass runs in the launches behind mcd_latent_reconstruct (mocodad_amd.engine.LatentReconstructor):
[condition encoder] -> encode -> [project] -> unproject -> decode.  3 or 5 .. 12 corrupt frames.

Reference: models/mocodad_latent.py, models/stsae/stsae_unet.py:254-438 (STSAE_Unet).  Training is outside the accelerated path.
"""
import argparse
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from .mocodad import UNetParams
from .mocodad_latent import LOSS_FNS, LatentStage


class LatentAEParams(UNetParams):
    """Parameter tree of STSAE_Unet with use_bottleneck (stsae_unet.py:254-363): the pose model's U-Net + to_time_dim onto the latent
    and rev_to_time_dim back."""

    def __init__(self, c_in: int, embedding_dim: int, latent_dim: int, n_frames: int, dropout: float):
        super().__init__(c_in, embedding_dim, n_frames, dropout)
        f = self.down_channels[6] * n_frames * 10
        self.to_time_dim = nn.Linear(f, latent_dim)
        self.rev_to_time_dim = nn.Linear(latent_dim, f)


class MoCoDADlatentPretrain(LatentStage):
    is_pretrain = True

    def __init__(self, args: argparse.Namespace) -> None:
        self.hidden_sizes = list(getattr(args, "hidden_sizes", None) or [])      # (a key of the YAML; the stage builds no denoiser)
        if args.stage != "pretrain":
            raise ValueError(f"MoCoDADlatentPretrain is the 'pretrain' stage of the latent model, got stage {args.stage!r}: "
                             "the 'diffusion' stage is mocodad_amd.models.mocodad_latent.MoCoDADlatent")
        super().__init__(args)
        self.model_return_value = "pose"      # (mocodad_latent.py:33)

    def build_model(self) -> None:
        super().build_model()
        self.model = LatentAEParams(self.num_coords, self.embedding_dim, self.latent_embedding_dim, self.n_frames_corrupt, self.dropout)
        self.eval()

    def build_scorer(self, device):
        """engine.LatentReconstructor with this module's weights (MoCoDAD.scorer() caches it per device)."""
        from ..engine import LatentReconstructor
        return LatentReconstructor(self.state_dict(), **self._scorer_kwargs(device))

    # -------------------------------------------------------------- forward
    def _corrupt_frames(self, tensor_data) -> torch.Tensor:
        """The corrupt frames of the batch, (B,C,t_corrupt,V): the second entry of forward's list (mocodad_latent.py:132)."""
        xi = self._frame_split()[1]
        if hasattr(tensor_data, "as_view"):
            tensor_data = tensor_data.materialize()
        return tensor_data[:, :, xi, :]

    def forward(self, input_data: List[torch.Tensor], condition_data: torch.Tensor = None, aggr_strategy: str = 'best', *,
                return_: str = None) -> List[torch.Tensor]:
        """[data (B,C,T,V), transformation_idx, metadata, actual_frames] -> [pose] + [corrupt frames, transformation_idx, metadata,
        actual_frames] as mocodad_latent.py:131-132 (`condition_data` and `aggr_strategy` are unused there too; the second entry
        is the CORRUPT frames, not the window).  Extension: return_='loss' gives the per-window mean reconstruction loss and 'all'
        [loss, pose], where the reference hands back None for the loss."""
        tensor_data, meta_out = self._unpack_data(input_data)
        ret = return_ if return_ is not None else self.model_return_value
        if ret not in ("pose", "loss", "all"):
            raise ValueError(f"Unknown return mode {ret}")
        pose, loss, _, _ = self.scorer().reconstruct(tensor_data, want_pose=ret != "loss", loss_fn=self.loss_name)
        return self._pack_out_data(pose, loss, [self._corrupt_frames(tensor_data)] + meta_out, return_=ret)

    def decode_latents(self, batch: List[torch.Tensor], latents: torch.Tensor) -> torch.Tensor:
        """The poses (B,C,t_corrupt,V) the decoder makes of the caller's (B,D) latents, with the batch's own skips and condition
        (rev_to_time_dim, the up path, + the corrupt frames): mcd_latent_reconstruct's z_in."""
        tensor_data, _ = self._unpack_data(batch)
        return self.scorer().reconstruct(tensor_data, latents.to(self.device), loss_fn=self.loss_name)[0]

    # -------------------------------------------------------------- test / validation loops: per-window losses stay on the device
    def test_step(self, batch, batch_idx: int) -> None:
        self._test_output_list.append(self._window_losses(batch))

    def validation_step(self, batch, batch_idx: int) -> None:
        self._validation_output_list.append(self._window_losses(batch))

    def _window_losses(self, batch) -> torch.Tensor:
        tensor_data, _ = self._unpack_data(batch)
        return self.scorer().reconstruct(tensor_data, want_pose=False, loss_fn=self.loss_name)[1]

    def _epoch_end(self, attr: str) -> float:
        """The reference's post_processing value (mocodad_latent.py:192-197, 218): every window has the same number of elements, so
        the mean of the window means, summed in float64, is the mean over all elements."""
        outs = getattr(self, attr)
        delattr(self, attr)
        if not outs:
            raise ValueError("no batches were scored")
        rec_loss = float(torch.cat([o.reshape(-1) for o in outs]).double().mean().item())
        self.last_scores = rec_loss
        self.log("pretrain_rec_loss", rec_loss)
        return rec_loss

    def post_processing(self, out, gt_data, trans=None, meta=None, frames=None) -> float:
        """mocodad_latent.py:217-218 on host arrays (saved tensors): mean loss_fn(out, gt_data)."""
        t = lambda a: a.detach().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
        return torch.mean(LOSS_FNS[self.loss_name](t(out), t(gt_data), reduction="none")).item()
