"""Test-time pose transforms of the reference's dataset (utils/dataset_utils.py:255-310, applied per item in
utils/dataset.py:67-76) as a small affine table, so that the HIP kernels can apply them while loading a window
instead of the host materialising num_transform copies of the dataset."""
import math

import numpy as np
import torch

# (sx, sy, tx, ty, rot_degrees, flip) of ae_trans_list, in order
AE_TRANSFORMS = [(1, 1, 0.0, 0.0, 0, False), (1, 1, 0.0, 0.0, 0, True), (1, 1, 0.0, 0.0, 90, False),
                 (1, 1, 0.0, 0.0, 90, True), (1, 1, 0.0, 0.0, 45, False)]


def affine_matrix(sx=1.0, sy=1.0, tx=0.0, ty=0.0, rot=0.0, flip=False) -> torch.Tensor:
    c, s = math.cos(math.radians(rot)), math.sin(math.radians(rot))
    flip_m = torch.diag(torch.tensor([-1.0 if flip else 1.0, 1.0, 1.0]))
    scale_m = torch.tensor([[sx, 0.0, tx], [0.0, sy, ty], [0.0, 0.0, 1.0]], dtype=torch.float32)
    rot_m = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    return flip_m @ (rot_m @ scale_m)


def affine_table(num_transform: int) -> torch.Tensor:
    """(num_transform, 6) fp32 rows [a00 a01 a02 a10 a11 a12]: x' = a00 x + a01 y + a02, y' = a10 x + a11 y + a12."""
    rows = [affine_matrix(*AE_TRANSFORMS[i])[:2].reshape(-1) for i in range(num_transform)]
    return torch.stack(rows).contiguous()


def inverse_affine_rows(affine) -> torch.Tensor:
    """(n, 6) affine rows -> (n, 6) float64 rows [i00 i01 i02 i10 i11 i12] of their inverses, x = i00 x' + i01 y' + i02,
    y = i10 x' + i11 y' + i12, in float64 from the values as given: det = a00 a11 - a01 a10; i00 = a11 / det, i01 = -a01 / det,
    i10 = -a10 / det, i11 = a00 / det; i02 = -(i00 a02 + i01 a12), i12 = -(i10 a02 + i11 a12).  A singular map is a ValueError.
    (Zeros come out as +0.0: the identity's row is (1, 0, 0, 0, 1, 0) in every bit.)"""
    a = (affine.detach().cpu().to(torch.float64).numpy() if torch.is_tensor(affine) else np.asarray(affine, np.float64)).reshape(-1, 6)
    out = []
    for k, (a00, a01, a02, a10, a11, a12) in enumerate(a):
        det = a00 * a11 - a01 * a10
        if det == 0 or det != det:
            raise ValueError(f"transform {k} is singular (determinant {det}): it has no inverse to map its forecasts back with")
        i00, i01, i10, i11 = a11 / det, -a01 / det, -a10 / det, a00 / det
        i02, i12 = -(i00 * a02 + i01 * a12), -(i10 * a02 + i11 * a12)
        out.append([v + 0.0 for v in (i00, i01, i02, i10, i11, i12)])
    return torch.tensor(out, dtype=torch.float64).reshape(-1, 6)


def inverse_affine_table(num_transform: int) -> torch.Tensor:
    """(num_transform, 6) float64: the inverses of the fp32 rows of affine_table, what maps a forecast made under transform t back
    to the coordinates of transform 0 (mcd_forecast_assemble_view, the stream's forecast ring of every transform)."""
    return inverse_affine_rows(affine_table(num_transform))
