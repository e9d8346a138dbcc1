"""Float64 torch restatement of the image tail (d3ga_amd/image_tail.py): torchvision's `gaussian_blur` (taps, sigma rule and
reflect padding recalled from torchvision, which is not part of the reference tree), the learnable blur of
models/learnable_blur.py:34-44 and the target composition of train.py:182-188.  The test oracle of the HIP kernels;
differentiable (autograd), any dtype / device the inputs have."""
import torch
import torch.nn.functional as F


def gaussian_taps(k, dtype=torch.float64, device=None):
    """g_k[i] ~ exp(-(x_i / sigma_k)^2 / 2), x_i = i - (k - 1) / 2, sigma_k = 0.15 k + 0.35, normalised to sum 1."""
    sigma = 0.15 * k + 0.35
    x = torch.linspace(-(k - 1) * 0.5, (k - 1) * 0.5, k, dtype=dtype, device=device)
    g = torch.exp(-0.5 * (x / sigma) ** 2)
    return g / g.sum()


def gaussian_blur_ref(img, kernel_size):
    """`torchvision.transforms.functional.gaussian_blur(img, kernel_size)` with its default sigma: img (..., C, H, W),
    kernel_size [kx, ky]; reflect padding of k // 2 (edge pixel not repeated), then a depth-wise conv2d with the outer
    product of the two tap vectors."""
    if isinstance(kernel_size, int):
        kernel_size = [kernel_size, kernel_size]
    kx, ky = int(kernel_size[0]), int(kernel_size[1])
    shape = img.shape
    x = img.reshape(-1, *shape[-3:])
    C = x.shape[1]
    k2 = torch.outer(gaussian_taps(ky, img.dtype, img.device), gaussian_taps(kx, img.dtype, img.device))
    x = F.pad(x, [kx // 2, kx // 2, ky // 2, ky // 2], mode="reflect")
    x = F.conv2d(x, k2.expand(C, 1, ky, kx), groups=C)
    return x.reshape(shape)


def learnable_blur_ref(img, weights_raw, cam_idx):
    """One image (C,H,W): softmax(weights_raw[cam_idx]) mix of img, B3(img), B7(img)."""
    w = torch.softmax(weights_raw[cam_idx], dim=-1)
    return w[0] * img + w[1] * gaussian_blur_ref(img, [3, 3]) + w[2] * gaussian_blur_ref(img, [7, 7])


def compose_target_ref(image, alpha, silhouette, boundary_fg, bg_color):
    """train.py:182-188, line by line (image (3,H,W), alpha (1,H,W), silhouette (3,H,W), boundary_fg (1,H,W), bg_color (3))."""
    dt = image.dtype
    gt_alpha = alpha.expand(3, -1, -1)
    gt_silhouette = silhouette * gt_alpha
    gt_image = image * gt_alpha + (1 - gt_alpha) * bg_color[:, None, None]
    boundary = 1. - boundary_fg.to(dt)
    gt_image = gt_image * boundary + (1. - boundary) * bg_color[:, None, None]
    gt_silhouette = gt_silhouette * boundary
    return gt_image, gt_silhouette
