#!/usr/bin/env python3
"""Generate the latent-path golden vectors by IMPORTING the reference's MoCoDADlatent on CPU.

Run where the reference checkout is (MOCODAD_REFERENCE, default /root/reference):   python tests/golden/gen_latent_golden.py

The reference class (models/mocodad_latent.py) is built in stage 'diffusion' with the Lightning stub of gen_golden.py and with
_freeze_main_net_and_load_ckpt patched out (the pretrain checkpoint it would read does not exist; a diffusion-stage state_dict
holds every tensor).  Weights are seeded random-init with perturbed BatchNorm statistics (BatchNorm1d included) and PReLU slopes;
the 'hostile' variant draws every BN gain log-uniform in 0.1x .. 10x and clips the windows to +-5.  The draws of torch.randn /
torch.randn_like are captured in call order (mocodad_latent.py:109,121) and stored in the layout the HIP path takes.

Only DATA is written: latent_<name>_w<part>.npz (the state_dict without the condition autoencoder's decoder, dead at evaluation; the
full sorted key / shape list; the YAML settings) and latent_<name>_io.npz (windows, draws, expected outputs)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import REF, _install_lightning_stub  # noqa: E402

AGGRS = ["best", "worst", "mean", "median", "quantile:0.3", "mean_pose", "median_pose"]
MAX_BYTES = 1 << 20      # no committed file above 1 MiB

#          name          weights      hostile D   hidden               ns  S  B   seed
CONFIGS = [("A_benign",  "A_benign",  False, 64, [64, 128, 128, 64], 10, 3, 37, 11),
           ("A_hostile", "A_hostile", True,  64, [64, 128, 128, 64], 10, 3, 37, 12),
           ("B",         "B",         False, 32, [48, 32],            2, 1, 5,  13),
           ("C",         "A_hostile", True,  64, [64, 128, 128, 64], 50, 2, 5,  14)]     # (C) shares (A) hostile's weights


def make_args(D, hidden, ns, S):
    cfg = yaml.load(open(os.path.join(REF, "config/UBnormal/mocodad-latent_test.yaml")), Loader=yaml.FullLoader)
    cfg.update(dict(latent_embedding_dim=D, hidden_sizes=list(hidden), noise_steps=ns, n_generated_samples=S, accelerator="cpu",
                    save_tensors=False, test_path="/tmp/none"))
    args = argparse.Namespace(**cfg)
    args.gt_path = args.test_path
    args.ckpt_dir = "/tmp/mocodad_golden_ckpt"
    return args, cfg


def perturb_(model, gen, hostile):
    for m in model.modules():
        if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) + 0.5)
            if hostile:
                m.weight.data.copy_(torch.exp((torch.rand(m.weight.shape, generator=gen) * 2 - 1) * np.log(10.0)))
            else:
                m.weight.data.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
        if isinstance(m, nn.PReLU):
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=gen) * 0.3 + 0.1)


class Capture:
    """Records what torch.randn / torch.randn_like return, in call order."""

    def __init__(self):
        self.draws = []
        self._randn, self._randn_like = torch.randn, torch.randn_like

    def __enter__(self):
        def randn(*a, **k):
            out = self._randn(*a, **k)
            self.draws.append(out.clone())
            return out

        def randn_like(x, **k):
            out = self._randn_like(x, **k)
            self.draws.append(out.clone())
            return out
        torch.randn, torch.randn_like = randn, randn_like
        return self

    def __exit__(self, *exc):
        torch.randn, torch.randn_like = self._randn, self._randn_like


def save(name, arrays):
    path = os.path.join(HERE, name)
    np.savez(path, **arrays)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{name}: {size} bytes"
    print(f"{name}: {size / 1024:.0f} KiB")


def main():
    _install_lightning_stub()
    sys.path.insert(0, REF)
    torch.set_grad_enabled(False)
    from models.mocodad_latent import MoCoDADlatent
    MoCoDADlatent._freeze_main_net_and_load_ckpt = lambda self: None
    models = {}
    for name, wname, hostile, D, hidden, ns, S, B, seed in CONFIGS:
        args, cfg = make_args(D, hidden, ns, S)
        gen = torch.Generator().manual_seed(seed)
        if wname not in models:
            torch.manual_seed(seed)
            m = MoCoDADlatent(args)
            m.eval()
            perturb_(m, gen, hostile)
            models[wname] = m
            sd = m.state_dict()
            keys = sorted([k, list(v.shape)] for k, v in sd.items())
            w = {k: v.numpy() for k, v in sd.items() if v.dtype.is_floating_point and not k.startswith(("condition_encoder.decoder.", "condition_encoder.rev_btlnk."))}
            w["__keys__"] = np.frombuffer(json.dumps(keys).encode(), dtype=np.uint8)
            w["__cfg__"] = np.frombuffer(json.dumps({k: v for k, v in cfg.items()}).encode(), dtype=np.uint8)
            # (in parts below the size limit for a committed file; the tests merge latent_<name>_w*.npz)
            parts, cur, size = [], {}, 0
            for k in sorted(w, key=lambda k: -w[k].nbytes):
                if cur and size + w[k].nbytes > 800 * 1024:
                    parts.append(cur)
                    cur, size = {}, 0
                cur[k] = w[k]
                size += w[k].nbytes
            parts.append(cur)
            for i, part in enumerate(parts):
                save(f"latent_{wname}_w{i}.npz", part)
        else:       # same weights, another schedule / sample count
            m = MoCoDADlatent(args)
            m.eval()
            m.load_state_dict(models[wname].state_dict())
        data = torch.randn(B, 2, 6, 17, generator=gen)
        if hostile:
            data = (data * 3).clamp(-5, 5)
        batch = [data, torch.zeros(B, dtype=torch.long), torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, 6, dtype=torch.int32)]
        torch.manual_seed(seed + 100)
        with Capture() as cap:
            loss_all, lat_all = m.forward(batch, aggr_strategy="all", return_="all")[:2]
        K = max(ns - 1, 1)
        assert len(cap.draws) == S * K, (len(cap.draws), S, K)
        noise = torch.stack(cap.draws).reshape(S, K, B, D)
        assert tuple(lat_all.shape) == (B, S, D) and tuple(loss_all.shape) == (B, S)
        cond_data, corrupt_data, idxs = m._select_frames(data)
        cond_emb, _ = m._encode_condition(cond_data)
        z0 = m._unet_forward(corrupt_data, t=torch.full((B,), -1, dtype=torch.long), condition_data=cond_emb, corrupt_idxs=idxs[1])
        out = {"data": data.numpy(), "noise": noise.numpy(), "cond_emb": cond_emb.numpy(), "z0": z0.numpy(),
               "latent_all": lat_all.numpy(), "loss_all": loss_all.numpy(),
               "sizes": np.array([D, ns, S, B], dtype=np.int64), "hidden": np.array(hidden, dtype=np.int64)}
        # Denoiser.forward alone, on the S*B rows of the x_T draws, at the first and the last step of the chain
        xr = noise[:, 0].reshape(S * B, D)
        cr = cond_emb.repeat(S, 1)
        for t in sorted({1, ns - 1}):
            out[f"eps_t{t}"] = m.denoiser(xr, torch.full((S * B,), t, dtype=torch.long), cr).numpy()
        gens = [lat_all[:, s] for s in range(S)]
        finite = bool(torch.isfinite(loss_all).all())
        for a in AGGRS:
            sel, loss = m._aggregation_strategy(gens, z0, a)
            tag = a.replace(":", "_")
            out[f"loss_{tag}"] = loss.numpy()
            if sel is not None:
                out[f"sel_{tag}"] = sel.numpy()
            finite = finite and bool(torch.isfinite(loss).all())
        assert finite, f"{name}: a recorded loss is not finite"
        print(f"{name}: loss_all in [{loss_all.min().item():.3e}, {loss_all.max().item():.3e}]  max|z0| {z0.abs().max().item():.3e}  "
              f"max|latent| {lat_all.abs().max().item():.3e}")
        save(f"latent_{name}_io.npz", out)


if __name__ == "__main__":
    main()
