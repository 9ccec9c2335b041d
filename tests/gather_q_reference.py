"""numpy side of the quantized gather (reduce_q with gather_format; DESIGN §3, include/edt_sync.h),
on top of tests/quant_reference.py: the wire format is that module's, unchanged; what is new is
what gets quantized — the owner's update u = f32(theta') - f32(theta) with its sharded residual —
and what every rank does with it, theta <- round(f32(theta) + D(q))."""
from __future__ import annotations

import numpy as np
import torch

from tests import quant_reference as Q


def _f32(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        return t.detach().float().cpu().numpy()
    return np.asarray(t, dtype=np.float32)


def delta_step(theta_old, theta_new, residual, fmt):
    """The owner's phase 2' after the SGD update: u = f32(theta_new) - f32(theta_old) (one fp32
    subtract), then ef_step: u' = u + r, q = Q(u'), r' = u' - D(q). residual None: no feedback.
    Returns (codes, scales, D(q), r' or None)."""
    with np.errstate(invalid="ignore"):
        u = (_f32(theta_new) - _f32(theta_old)).astype(np.float32)
    return Q.ef_step(u, residual, fmt)


def apply_delta(theta: torch.Tensor, d) -> torch.Tensor:
    """Phase 3: round(f32(theta) + D(q)) to theta's dtype (one fp32 add, then RNE); a new tensor."""
    d = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).to(theta.device)
    return (theta.float() + d).to(theta.dtype)


class NumpyGatherKernels(Q.NumpyQuantKernels):
    """NumpyQuantKernels plus the two entries of the quantized gather, on CPU tensors."""

    def sgd_delta_sum_q(self, theta, regions, fmt_in, momentum, has_momentum, lr, mu, nesterov, packed_out, fmt_out,
                        residual=None):
        new = theta.clone()
        self.sgd_apply_sum_q(new, regions, fmt_in, momentum, has_momentum, lr, mu, nesterov)
        codes, scales, _, r = delta_step(theta, new, None if residual is None else residual.numpy(), fmt_out)
        if residual is not None:
            residual.copy_(torch.from_numpy(r))
        packed_out.copy_(torch.from_numpy(Q.pack(codes, scales, fmt_out, theta.numel())))

    def apply_delta_q(self, theta, packed, region_elems, fmt):
        d = Q.dequantize(*Q.unpack(packed.numpy(), fmt, region_elems), fmt)
        theta.copy_(apply_delta(theta, d))
