"""pytorch3d.utils.cameras_from_opencv_projection (recorder/pc_renderer.py:10,54, lib/segmentation.py:21,45)."""
import torch

from .renderer import PerspectiveCameras

__all__ = ["cameras_from_opencv_projection"]


def cameras_from_opencv_projection(R, tvec, camera_matrix, image_size):
    """R (N,3,3), tvec (N,3), camera_matrix (N,3,3), image_size (N,2) as (height, width) rows -> PerspectiveCameras: OpenCV's
    x_cam = R x + tvec, u = fx x/z + cx, v = fy y/z + cy.  Works on CPU tensors; nothing touches the GPU before the first
    rasterization."""
    what = "cameras_from_opencv_projection"
    for name, t, tail in (("R", R, (3, 3)), ("tvec", tvec, (3,)), ("camera_matrix", camera_matrix, (3, 3)), ("image_size", image_size, (2,))):
        if not torch.is_tensor(t) or t.dim() != len(tail) + 1 or tuple(t.shape[1:]) != tail:
            raise ValueError(f"{what}: expected {name} (N,{','.join(map(str, tail))}), got {tuple(getattr(t, 'shape', ()))}")
    N = R.shape[0]
    if not (tvec.shape[0] == camera_matrix.shape[0] == image_size.shape[0] == N):
        raise ValueError(f"{what}: R, tvec, camera_matrix and image_size hold different numbers of cameras")
    return PerspectiveCameras(_opencv=(R, tvec, camera_matrix, image_size))
