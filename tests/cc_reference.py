"""The reference of the colour-corrected metrics' tests (tests/test_eval_cc_cpu.py, tests/test_eval_cc_gpu.py): the
definition of include/gr_hip.h restated in float64 numpy on the float32-rounded inputs: the 22 moments, the ridge solve
by Cholesky, the affine apply and the three metrics (the SSIM from tests/ssim_reference.py's dense evaluation)."""
from __future__ import annotations

import numpy as np
import torch

import ssim_reference as ref

RIDGE = 1e-6  # GR_CC_RIDGE
IDENTITY = np.eye(3, 4)


def _f64(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.astype(np.float64)


def moments(x, t):
    """A = sum u u^T (4, 4) and B = sum u t^T (4, 3) over all pixels, u = (x0, x1, x2, 1)."""
    x, t = _f64(x).reshape(-1, 3), _f64(t).reshape(-1, 3)
    u = np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)
    return u.T @ u, u.T @ t


def solve(A, B, hw: int, ridge: float = RIDGE) -> np.ndarray:
    """E (3, 4) float64: row k solves (A / HW + ridge I) E_k^T = B[:, k] / HW + ridge e_k."""
    M = A / hw + ridge * np.eye(4)
    R = B / hw + ridge * np.eye(4, 3)
    L = np.linalg.cholesky(M)
    z = np.linalg.solve(L, R)
    return np.linalg.solve(L.T, z).T


def fit(x, t, ridge: float = RIDGE) -> np.ndarray:
    """The transform as the implementations return it: float64 solve, rounded to float32 once."""
    A, B = moments(x, t)
    return solve(A, B, _f64(x).reshape(-1, 3).shape[0], ridge).astype(np.float32)


def apply(x, E) -> np.ndarray:
    """E (x, 1) in float64 (the implementations round every operation to float32: within a few 1e-7 of this)."""
    E = _f64(E).reshape(3, 4)
    return _f64(x) @ E[:, :3].T + E[:, 3]


def metrics(x, t, E=None) -> dict:
    """l1, mse, ssim of E (x, 1) (E None: of x) against t, in float64."""
    y, t = (_f64(x) if E is None else apply(x, E)), _f64(t)
    d = y - t
    return {"l1": float(np.abs(d).mean()), "mse": float((d * d).mean()),
            "ssim": 1.0 - float(ref.dssim_dense(torch.from_numpy(y), torch.from_numpy(t)))}
