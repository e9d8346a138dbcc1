"""pytorch3d.transforms.matrix_to_quaternion (lib/cage.py:18,290, lib/batch.py:18, models/garment_net.py:187): a torch
restatement.  It runs per frame on one 3 x 3 and once at construction, so no kernel is warranted, and autograd comes free.
Works on any device and dtype."""
import torch

__all__ = ["matrix_to_quaternion"]


def _sqrt_positive_part(x):
    """sqrt(max(0, x)) with a zero (sub)gradient where x <= 0"""
    pos = x > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))


def matrix_to_quaternion(matrix):
    """Rotation matrices (..., 3, 3) -> quaternions (..., 4), real part first and non-negative.

    q_abs = sqrt(max(0, .)) of [1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22] are twice the
    magnitudes of (r, i, j, k); each gives one candidate quaternion (the one whose dominant component it is), divided by
    2 max(q_abs_k, 0.1); the candidate of the largest q_abs is taken -- the four q_abs^2 sum to 4, so that one is >= 1 and
    nothing is amplified -- and standardized to a non-negative real part."""
    if not torch.is_tensor(matrix) or matrix.dim() < 2 or tuple(matrix.shape[-2:]) != (3, 3):
        raise ValueError(f"matrix_to_quaternion: expected (..., 3, 3), got {tuple(getattr(matrix, 'shape', ()))}")
    batch = matrix.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(matrix.reshape(batch + (9,)), dim=-1)
    q_abs = _sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22,
                                             1.0 - m00 - m11 + m22], dim=-1))
    by_rijk = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1),
    ], dim=-2)
    candidates = by_rijk / (2.0 * q_abs[..., None].clamp_min(0.1))
    pick = q_abs.argmax(dim=-1)[..., None, None].expand(batch + (1, 4))
    q = torch.gather(candidates, -2, pick).squeeze(-2)
    return torch.where(q[..., 0:1] < 0, -q, q)
