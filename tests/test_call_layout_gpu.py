"""GPU: the workspace of a scoring call -- what the sizing entries report, and that a call stays inside it.

(a) mcd_score_workspace_bytes, mcd_pass_workspace_bytes, mcd_plan_split and mcd_latent_workspace_bytes for B in {1, 3, 37, 1024},
    S in {1, 5, 50} equal tests/golden/call_layout.json, recorded on the MI355X from the library before the call front end
    (mcd_call.hpp) existed:  python tests/test_call_layout_gpu.py --record
(b) a call given exactly the reported bytes, followed by 256 guard bytes, leaves the guard intact and writes bit for bit what
    the same call writes into a workspace 1 MB larger: no region is carved past what the sizing entry counted."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN  # noqa: E402
from test_call_errors_gpu import _ptr, make_cfg  # noqa: E402

pytestmark = pytest.mark.gpu
JSON = os.path.join(GOLDEN, "call_layout.json")
BS, SS, NS = [1, 3, 37, 1024], [1, 5, 50], 10
POSE = ["inject", "concat", "T12", "seg20", "cat24", "encU", "inject+cond_generic"]
LATENT = ["A_benign", "B", "U", "G", "C7"]
_cache = {}


def pose(name):
    if name not in _cache:
        from helpers import golden_weights
        from mocodad_amd.engine import HipScorer
        from oracle import mocodad_oracle as O
        variant, _, opt = name.partition("+")
        sd, cfg = golden_weights(variant)
        strat = cfg["conditioning_strategy"]
        ci, xi = O.split_indices(cfg["seg_len"], cfg["conditioning_indices"], strat)
        unet = cfg["conditioning_architecture"] == "E_unet"
        _cache[name] = HipScorer(sd, strategy=strat, seg_len=cfg["seg_len"], cond_idx=ci, corrupt_idx=xi, cond_unet=unet,
                                 cond_channels=[] if unet else list(cfg["channels"]) + [cfg["h_dim"]], device="cuda:0",
                                 options={opt: 1} if opt else None)
    return _cache[name]


def latent(name):
    if name not in _cache:
        import latent_ref as R
        import latentx_fixtures as X
        from helpers import make_args
        from mocodad_amd.models.mocodad_latent import MoCoDADlatent
        sd, _, cfg, _ = X.load(name) if name in X.NAMES else R.load_fixture(name)
        m = MoCoDADlatent(make_args(cfg))
        m.load_state_dict(sd, strict=False)
        _cache[name] = m.to("cuda:0").scorer()
    return _cache[name]


class _Of:      # (make_cfg takes an object with .sc)
    def __init__(self, sc):
        self.sc = sc


def sizes_of(name):
    """What the sizing entries report for one handle: {call: bytes or split}."""
    if name.startswith("latent "):
        sc = latent(name[len("latent "):])
        return {f"B={b}": int(sc.L.mcd_latent_workspace_bytes(sc._h, b)) for b in BS}
    sc = pose(name)
    rows = {}
    for b in BS:
        rows[f"pass B={b}"] = int(sc.L.mcd_pass_workspace_bytes(sc._h, b))
        for s in SS:
            cfg = make_cfg(_Of(sc), B=b, S=s, ns=NS)
            rows[f"score B={b} S={s}"] = int(sc.L.mcd_score_workspace_bytes(sc._h, C.byref(cfg)))
            rows[f"split B={b} S={s}"] = int(sc.L.mcd_plan_split(sc._h, C.byref(cfg)))
    return rows


HANDLES = POSE + ["latent " + n for n in LATENT]


@pytest.fixture(scope="module")
def recorded():
    with open(JSON) as f:
        return json.load(f)


@pytest.mark.parametrize("name", HANDLES)
def test_sizing_entries(name, recorded):
    assert sizes_of(name) == recorded["sizes"][name]


# ---- (b)
B, S, NSB, GUARD, PATTERN = 3, 2, 4, 256, 0xA5


def _workspace(need, extra):
    """need + extra bytes; the bytes behind `need` hold PATTERN (the first GUARD of them are checked)."""
    ws = torch.full((need + max(extra, GUARD),), PATTERN, dtype=torch.uint8, device="cuda:0")
    ws[:need] = 0x5A        # (not zero: a region the call relies on must be written by the call)
    return ws


def _pose_call(sc, ws):
    gen = torch.Generator().manual_seed(3)
    data = torch.randn(B, 2, sc.seg_len, 17, generator=gen).cuda()
    noise = torch.randn(S, NSB - 1, B, 2, len(sc.corrupt_idx), 17, generator=gen).cuda()
    agg = torch.full((B,), -7.0, device="cuda:0")
    cfg = make_cfg(_Of(sc), B=B, S=S, ns=NSB)
    rc = sc.L.mcd_score_fused(sc._h, C.byref(cfg), _ptr(data), None, _ptr(noise), 0, 0, _ptr(sc.table(NSB)), _ptr(ws), 1, C.c_float(0.0),
                              _ptr(agg), None, None, None)       # aggregation best, loss_all = NULL: the loss region is live
    assert rc == 0, sc.L.mcd_last_error().decode()
    torch.cuda.synchronize()
    return [agg]


def _latent_call(sc, ws):
    gen = torch.Generator().manual_seed(3)
    D = sc.latent_dim
    data = torch.randn(B, 2, sc.seg_len, 17, generator=gen).cuda()
    noise = torch.randn(S, NSB - 1, B, D, generator=gen).cuda()
    agg, loss = torch.full((B,), -7.0, device="cuda:0"), torch.full((B, S), -7.0, device="cuda:0")
    lat, code = torch.full((B, S, D), -7.0, device="cuda:0"), torch.full((B, D), -7.0, device="cuda:0")
    cfg = make_cfg(_Of(sc), B=B, S=S, ns=NSB)
    rc = sc.L.mcd_latent_score(sc._h, C.byref(cfg), _ptr(data), None, _ptr(noise), 0, 0, _ptr(sc.table(NSB)), _ptr(ws), 1, C.c_float(0.0),
                               _ptr(agg), _ptr(loss), _ptr(lat), _ptr(code), None)
    assert rc == 0, sc.L.mcd_last_error().decode()
    torch.cuda.synchronize()
    return [agg, loss, lat, code]


def _need(sc, is_latent):
    if is_latent:
        return int(sc.L.mcd_latent_workspace_bytes(sc._h, B))
    cfg = make_cfg(_Of(sc), B=B, S=S, ns=NSB)
    return int(sc.L.mcd_score_workspace_bytes(sc._h, C.byref(cfg)))


@pytest.mark.parametrize("case", ["inject cond_generic split=2", "inject cond_generic split=2 generic_unet", "latent G"])
def test_call_stays_inside_the_reported_workspace(case, recorded):
    is_latent = case.startswith("latent")
    if is_latent:
        sc, opts, call = latent("G"), {}, _latent_call
    else:
        sc, call = pose("inject"), _pose_call
        opts = {"cond_generic": 1, "split": 2, **({"generic_unet": 1} if "generic_unet" in case else {})}
    for k, v in opts.items():
        sc.set_option(k, v)
    try:
        need = _need(sc, is_latent)
        assert need == recorded["call_bytes"][case]
        assert need > 0 and need % 256 == 0
        tight = _workspace(need, 0)
        got = call(sc, tight)
        assert bool((tight[need:need + GUARD] == PATTERN).all()), "the call wrote behind the bytes the sizing entry reported"
        roomy = _workspace(need, 1 << 20)
        ref = call(sc, roomy)
        assert bool((roomy[need:] == PATTERN).all())
        for g, r in zip(got, ref):
            assert bool((r != -7.0).all())          # (every output element was written)
            assert torch.equal(g, r)
    finally:
        for k in opts:
            sc.set_option(k, 0)


def call_bytes():
    out = {}
    sc = pose("inject")
    for case, opts in (("inject cond_generic split=2", {"cond_generic": 1, "split": 2}),
                       ("inject cond_generic split=2 generic_unet", {"cond_generic": 1, "split": 2, "generic_unet": 1})):
        for k, v in opts.items():
            sc.set_option(k, v)
        out[case] = _need(sc, False)
        for k in opts:
            sc.set_option(k, 0)
    out["latent G"] = _need(latent("G"), True)
    return out


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], __doc__
    how = ("`python tests/test_call_layout_gpu.py --record` on the MI355X with the library built from the commit before the call "
           "front end (mcd_call.hpp); noise_steps 10 for the sizing table")
    with open(sys.argv[2] if len(sys.argv) > 2 else JSON, "w") as f:
        json.dump({"how": how, "sizes": {n: sizes_of(n) for n in HANDLES}, "call_bytes": call_bytes()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded")
