"""pytorch3d.common.compat.meshgrid_ij (recorder/pc_renderer.py:19)."""
import torch

__all__ = ["meshgrid_ij"]


def meshgrid_ij(*tensors):
    """torch.meshgrid(..., indexing="ij"); a single list or tuple of tensors is accepted as torch.meshgrid accepts it."""
    if len(tensors) == 1 and isinstance(tensors[0], (list, tuple)):
        tensors = tuple(tensors[0])
    return torch.meshgrid(*tensors, indexing="ij")
