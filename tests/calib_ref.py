"""Float64 restatement of the per-camera colour calibration and pixel bias (d3ga_amd/calibration.py), the test oracle of
csrc/calib.hip:
  * the affine map out = rgb * w + b with (w, b) = corrections[cam][:3], [3:], views of the identity camera passed through,
    with its gradients written out (no autograd): dL/drgb = g w, dL/dcorrections[cam] = grad_scale (sum g rgb | sum g) per
    channel, summed over the views of a camera, zero rows for every other camera and for the identity camera;
  * bilinear upsampling by the rule of F.interpolate(mode='bilinear', align_corners=False) as one matrix per axis, U (n_out,
    n_in): up(B) = U_h B U_w^T, and its adjoint U_h^T G U_w.
numpy, float64 throughout."""
import numpy as np


def color_calib_ref(rgb, corrections, cams, identity_idx=None, channels_first=False):
    """rgb (k,P,3), or (k,3,...) with channels_first; cams: k indices -> out, same shape."""
    rgb = np.asarray(rgb, np.float64)
    cor = np.asarray(corrections, np.float64)
    out = np.empty_like(rgb)
    for v, c in enumerate(cams):
        if identity_idx is not None and c == identity_idx:
            out[v] = rgb[v]
            continue
        w, b = cor[c, :3], cor[c, 3:]
        if channels_first:
            shape = (3,) + (1,) * (rgb.ndim - 2)
            out[v] = rgb[v] * w.reshape(shape) + b.reshape(shape)
        else:
            out[v] = rgb[v] * w + b
    return out


def color_calib_grads_ref(rgb, corrections, cams, g, identity_idx=None, channels_first=False, grad_scale=1.0):
    """-> (dL/drgb, dL/dcorrections (n_cameras,6)) for the upstream gradient g (the shape of rgb)."""
    rgb, g = np.asarray(rgb, np.float64), np.asarray(g, np.float64)
    cor = np.asarray(corrections, np.float64)
    g_rgb, g_cor = np.empty_like(rgb), np.zeros_like(cor)
    for v, c in enumerate(cams):
        if identity_idx is not None and c == identity_idx:
            g_rgb[v] = g[v]
            continue
        w = cor[c, :3]
        if channels_first:
            g_rgb[v] = g[v] * w.reshape((3,) + (1,) * (rgb.ndim - 2))
            axes = tuple(range(1, rgb.ndim - 1))
            g_cor[c, :3] += grad_scale * (g[v] * rgb[v]).sum(axis=axes)
            g_cor[c, 3:] += grad_scale * g[v].sum(axis=axes)
        else:
            g_rgb[v] = g[v] * w
            g_cor[c, :3] += grad_scale * (g[v] * rgb[v]).reshape(-1, 3).sum(axis=0)
            g_cor[c, 3:] += grad_scale * g[v].reshape(-1, 3).sum(axis=0)
    return g_rgb, g_cor


def axis_coords(n_in, n_out):
    """Per output sample of one axis: (src, i0, i1, lambda) with src = max(0, (dst + 0.5) n_in / n_out - 0.5), i0 = floor(src),
    i1 = min(i0 + 1, n_in - 1), lambda = src - i0."""
    dst = np.arange(n_out, dtype=np.float64)
    src = np.maximum(0.0, (dst + 0.5) * (float(n_in) / float(n_out)) - 0.5)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return src, i0, i1, src - i0


def interp_matrix(n_in, n_out):
    """U (n_out, n_in): row dst holds 1 - lambda at i0 and lambda at i1 (both on one cell where i1 == i0)."""
    _, i0, i1, lam = axis_coords(n_in, n_out)
    U = np.zeros((n_out, n_in), np.float64)
    rows = np.arange(n_out)
    np.add.at(U, (rows, i0), 1.0 - lam)
    np.add.at(U, (rows, i1), lam)
    return U


def cell_ranges(n_in, n_out):
    """Per low-resolution cell i the half-open range [lo, hi) of output samples that can touch it: i - 1 <= i0(dst) <= i
    (i0 is non-decreasing, so this is one run)."""
    _, i0, _, _ = axis_coords(n_in, n_out)
    lo = np.searchsorted(i0, np.arange(n_in) - 1, side="left")
    hi = np.searchsorted(i0, np.arange(n_in), side="right")
    return np.stack([lo, hi], 1)


def pixel_bias_ref(bias_map, H, W):
    """bias_map (h,w) -> its upsampled map (H,W)."""
    B = np.asarray(bias_map, np.float64)
    return interp_matrix(B.shape[0], H) @ B @ interp_matrix(B.shape[1], W).T


def pixel_bias_grad_ref(g, h, w):
    """g (C,H,W) or (H,W): upstream gradient of the (broadcast) upsampled map -> dL/dbias_map (h,w) = U_h^T (sum_c g_c) U_w."""
    G = np.asarray(g, np.float64)
    if G.ndim == 3:
        G = G.sum(0)
    return interp_matrix(h, G.shape[0]).T @ G @ interp_matrix(w, G.shape[1])
