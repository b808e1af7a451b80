"""Kernel descriptors of the SVGD update.  The engine evaluates them on the device (k_kmat in
dibs_amd/csrc/kernels_marginal.h); these classes carry the hyper-parameters and offer a host ``eval`` for
inspection.  Reference: dibs/kernel.py:4-30 (AdditiveFrobeniusSEKernel), :33-71 (JointAdditive...).

Beyond the reference: a bandwidth may be the string ``"median"`` -- the median heuristic of Liu & Wang (2016),
``h = median ||x_a - x_b||^2 / log(M + 1)`` over the M particles of a run, selected on the device in every step
(include/dibs_hip.h, MEDIAN-HEURISTIC KERNEL BANDWIDTH).  ``median_bandwidth`` is its definition on the host."""
import math

import numpy as np

from ._abi import MEDIAN

_FLT_MIN = np.finfo(np.float32).tiny


def _check_bandwidth(name, h):
    if isinstance(h, str) and h != MEDIAN:
        raise ValueError(f"{name} must be a number or {MEDIAN!r}, got {h!r}")
    return h


def _no_pair_median(name):
    raise ValueError(f"{name}={MEDIAN!r}: the bandwidth is the median over all pairs of a run's particles, which a single pair does not "
                     "have; dibs_amd.kernel.median_bandwidth(x) gives it for a set of particles")


def median_bandwidth(x, batch_dims=0):
    """The median-rule bandwidth of the particles ``x`` ``[M, ...]`` (trailing axes are one particle, flattened), as the engine defines it:

    ``v_ab`` = float32 of the float64 sum of squared differences of particles a and b; ``med`` = the median of the ``P = M (M - 1) / 2``
    values with ``a < b`` -- P odd: the order statistic ``(P - 1) / 2``; P even: ``0.5f * (v[P/2 - 1] + v[P/2])`` in float32;
    ``h = max(float32(float64(med) * (1 / log(M + 1))), FLT_MIN)``.  Returns a float32 scalar.

    ``batch_dims`` = n: ``x`` is ``[b_1, ..., b_n, M, ...]``, one run per leading index; returns float32 ``[b_1, ..., b_n]``."""
    x = np.asarray(x, np.float64)
    if batch_dims:
        lead = x.shape[:batch_dims]
        runs = x.reshape((-1,) + x.shape[batch_dims:])
        return np.array([median_bandwidth(r) for r in runs], np.float32).reshape(lead)
    M = x.shape[0]
    if M < 2:
        raise ValueError("median_bandwidth needs at least two particles")
    x = x.reshape(M, -1)
    iu = np.triu_indices(M, 1)
    v = np.sort(((x[iu[0]] - x[iu[1]]) ** 2).sum(-1).astype(np.float32))
    P = v.size
    med = v[(P - 1) // 2] if P % 2 else np.float32(0.5) * (v[P // 2 - 1] + v[P // 2])
    h = np.float32(np.float64(med) * (1.0 / math.log(M + 1)))   # (the C library's log, as the engine's host side)
    return np.float32(max(h, _FLT_MIN))


class AdditiveFrobeniusSEKernel:
    def __init__(self, *, h=20.0, scale=1.0):
        self.h = _check_bandwidth("h", h)
        self.scale = scale

    def eval(self, *, x, y):
        if self.h == MEDIAN:
            _no_pair_median("h")
        return self.scale * np.exp(-np.sum((np.asarray(x) - np.asarray(y)) ** 2.0) / self.h)


class JointAdditiveFrobeniusSEKernel:
    def __init__(self, *, h_latent=5.0, h_theta=500.0, scale_latent=1.0, scale_theta=1.0):
        self.h_latent = _check_bandwidth("h_latent", h_latent)
        self.h_theta = _check_bandwidth("h_theta", h_theta)
        self.scale_latent = scale_latent
        self.scale_theta = scale_theta

    def eval(self, *, x_latent, x_theta, y_latent, y_theta):
        from .utils.tree import tree_leaves
        for name in ("h_latent", "h_theta"):
            if getattr(self, name) == MEDIAN:
                _no_pair_median(name)
        zn = np.sum((np.asarray(x_latent) - np.asarray(y_latent)) ** 2.0)
        tn = sum(np.sum((a - b) ** 2.0) for a, b in zip(tree_leaves(x_theta), tree_leaves(y_theta)))
        return self.scale_latent * np.exp(-zn / self.h_latent) + self.scale_theta * np.exp(-tn / self.h_theta)
