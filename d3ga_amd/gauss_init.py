"""Gaussian initialisation (csrc/gauss_init.hip): from a body mesh with part labels to the tensors a `CageNet`
starts from -- reproducible from a seed, with no trimesh, no pytorch3d and no pass through the host.

    lib/cage.py:166-239   CageBase.sample_body_surface (the masks and their order)         body_surface_draws
    lib/cage.py:241-260   CageBase.compute_tris_bary                                       sample_surface (.barys)
    lib/cage.py:262-296   CageBase.sample_initial_points                                   sample_initial_points
    lib/cage.py:271-272   mesh.vertex_normals * inflate (trimesh: angle-weighted)           inflate, vertex_normals_angle
    models/cage_net.py:57-77  the parameter block of CageNet.__init__                       init_cage_parameters

The rules are pinned by csrc/gauss_init_math.h, whose g++ build gives the kernels' bits, and against the reference's own
`sample_initial_points` run on recorded uniforms (tests/golden/gauss_init_cases.npz).  The arithmetic is float64 with one rounding
to float32 per output element, as the reference's numpy / torch float64 followed by `.float()`.  Face weights are integers (areas
scaled by a power of two and floored), so their prefix sum is exact and a draw depends on the uniforms alone -- not on the launch
geometry, not on scheduling.  The uniforms are an input: `torch.rand((n, 3), float64)` from a device generator seeded with `seed`
unless given.  Parity with numpy's random stream, with trimesh and with pytorch3d is unpinned.

One departure from the reference: `sample_body_surface` also draws `n_intsec_gaussians` samples on the ring where garments meet
the body and then throws them away (the lines that would add them are commented out there).  They are not drawn here.

Forward only, no gradient.  GPU tensors only; no kernel launch synchronises with the host (`check()` and the validation of face
indices read back, once each)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import D3GAError, check, dptr, require_cuda, stream_handle
from .mesh_render import MeshTopology

__all__ = ["SurfaceSamples", "sample_surface", "vertex_normals_angle", "inflate", "body_surface_draws", "sample_initial_points",
           "init_cage_parameters"]

_FIELDS = (("points", 3, torch.float32), ("rotations", 4, torch.float32), ("faces", 3, torch.int32), ("face_id", 0, torch.int32),
           ("barys", 3, torch.float32))


class SurfaceSamples:
    """What `sample_surface` writes: points (n,3) f32, rotations (n,4) f32 wxyz, faces (n,3) int32 (the vertices of each sample's
    face), face_id (n) int32 (its index in the ORIGINAL face list), barys (n,3) f32 -- and the sticky status word of the draws
    that wrote into it.  `rows(a, b)` is a view of rows a..b that shares the status; `check()` reads it back."""

    def __init__(self, points, rotations, faces, face_id, barys, status):
        self.points, self.rotations, self.faces, self.face_id, self.barys, self.status = points, rotations, faces, face_id, barys, status

    @classmethod
    def empty(cls, n, device="cuda"):
        n = int(n)
        if n < 1:
            raise ValueError(f"SurfaceSamples.empty: n = {n}, expected at least 1")
        t = [torch.empty((n, c) if c else (n,), dtype=dt, device=device) for _, c, dt in _FIELDS]
        return cls(*t, torch.zeros(1, dtype=torch.int32, device=device))

    def __len__(self):
        return self.points.shape[0]

    def __iter__(self):
        return iter((self.points, self.rotations, self.faces, self.face_id, self.barys))

    def rows(self, a, b):
        a, b = int(a), int(b)
        if not 0 <= a < b <= len(self):
            raise ValueError(f"SurfaceSamples.rows: [{a}, {b}) is no range of rows of {len(self)}")
        return SurfaceSamples(*(t[a:b] for t in self), self.status)

    def check(self):
        """One read-back: raises ValueError if a draw had nothing to sample from (every face masked out, degenerate or far below
        the largest) or met a face that names a vertex outside the mesh."""
        s = int(self.status.item())
        if s & _lib.SAMPLE_STATUS_RANGE:
            raise ValueError("sample_surface: a face names a vertex outside [0, V)")
        if s & _lib.SAMPLE_STATUS_EMPTY:
            raise ValueError("sample_surface: nothing to sample from: every face has weight 0 (masked out or without area)")
        return self


def _same_device(a, b):
    a, b = torch.device(a), torch.device(b)
    return a.type == b.type and (a.index == b.index or a.index is None or b.index is None)


def _as_tensor(what, name, x, device=None):
    if torch.is_tensor(x):
        return x.detach()
    if isinstance(x, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(x))
        if device is None:
            device = "cuda"
        if torch.device(device).type == "cuda" and not torch.cuda.is_available():
            raise D3GAError("d3ga_amd ops run on the GPU only and no GPU is available; there is no CPU fallback")
        return t.to(device)
    raise ValueError(f"{what}: {name} must be a tensor or an array, got {type(x).__name__}")


def _mesh(what, vertices, faces):
    """-> (vertices (V,3) float64 contiguous, faces (F,3) int32 contiguous) on the vertices' device; converted once"""
    v = _as_tensor(what, "vertices", vertices)
    if v.dim() == 3 and v.shape[0] == 1:
        v = v[0]
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError(f"{what}: expected vertices (V,3) with V >= 1, got {tuple(v.shape)}")
    if v.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: vertices must be float32 or float64, got {v.dtype}")
    if v.shape[0] > (2 ** 31 - 1) // 3:
        raise ValueError(f"{what}: 3 V must stay below 2^31, got V = {v.shape[0]}")
    if isinstance(faces, MeshTopology):
        faces = faces.faces(v.device)
    f = _as_tensor(what, "faces", faces, v.device)
    if f.dim() == 3 and f.shape[0] == 1:
        f = f[0]
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"{what}: expected faces (F,3), got {tuple(f.shape)}")
    if f.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: faces must be int32 or int64, got {f.dtype}")
    if not 1 <= f.shape[0] < _lib.SAMPLE_MAX_FACES:
        raise ValueError(f"{what}: F = {f.shape[0]} outside 1 .. 2^24 - 1")
    if not _same_device(f.device, v.device):
        raise ValueError(f"{what}: faces are on {f.device}, vertices on {v.device}")
    if f.device.type != "meta":
        lo, hi = int(f.min()), int(f.max())
        if lo < 0 or hi >= v.shape[0]:
            raise ValueError(f"{what}: faces name vertex {lo if lo < 0 else hi}, there are {v.shape[0]}")
    return v.to(torch.float64).contiguous(), f.to(torch.int32).contiguous()


def _check_out(what, out, n, device):
    if isinstance(out, (tuple, list)) and len(out) == 5:
        out = SurfaceSamples(*out, torch.zeros(1, dtype=torch.int32, device=device))
    if not isinstance(out, SurfaceSamples):
        raise ValueError(f"{what}: out must be a SurfaceSamples or its five tensors, got {type(out).__name__}")
    for (name, c, dt), t in zip(_FIELDS, out):
        want = (n, c) if c else (n,)
        if not torch.is_tensor(t) or tuple(t.shape) != want or t.dtype != dt or not t.is_contiguous() or not _same_device(t.device, device):
            raise ValueError(f"{what}: out.{name} must be a contiguous {dt} tensor {want} on {device}, got "
                             f"{(tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__}")
    s = out.status
    if not torch.is_tensor(s) or s.numel() != 1 or s.dtype != torch.int32 or not _same_device(s.device, device):
        raise ValueError(f"{what}: out.status must be one int32 on {device}")
    return out


def sample_surface(vertices, faces, n, *, face_mask=None, uniforms=None, seed=None, out=None, block=0):
    """n area-weighted samples of a triangle mesh -> SurfaceSamples.

    vertices (V,3) float64 (float32 is converted once), faces (F,3) int32 (int64 is converted once), F < 2^24.
    face_mask (F) bool or uint8: the faces to sample from (default all); `face_id` indexes the ORIGINAL face list either way.
    uniforms (n,3) float64 in [0,1): column 0 picks the face, columns 1 and 2 the point.  Default: `torch.rand((n,3), float64)`
    from a device generator seeded with `seed` (seed None: the device's default generator).
    out: a SurfaceSamples (or a `.rows(a, b)` view of one) of n rows to write into, so several draws share one buffer.
    block: lanes per workgroup of the per-sample launch (0: 256); the results do not depend on it.
    A face of weight 0 -- masked out, degenerate, or below 2^-(62 - ceil(log2 F)) of the power of two above the largest area --
    is never chosen.  With nothing to sample from the status word is set (`.check()` raises), the rows are zeros and face_id -1."""
    what = "sample_surface"
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise ValueError(f"{what}: n must be an integer, got {type(n).__name__}")
    n = int(n)
    if not 1 <= n <= (2 ** 31 - 1) // 4:
        raise ValueError(f"{what}: n = {n} outside 1 .. {(2 ** 31 - 1) // 4}")
    if block not in (0, 64, 128, 256, 512, 1024):
        raise ValueError(f"{what}: block = {block!r}, expected 0, 64, 128, 256, 512 or 1024")
    v, f = _mesh(what, vertices, faces)
    V, F, dev = v.shape[0], f.shape[0], v.device
    mask = None
    if face_mask is not None:
        mask = _as_tensor(what, "face_mask", face_mask, dev)
        if mask.dim() != 1 or mask.shape[0] != F:
            raise ValueError(f"{what}: expected face_mask ({F},), got {tuple(mask.shape)}")
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"{what}: face_mask must be bool or uint8, got {mask.dtype}")
        if not _same_device(mask.device, dev):
            raise ValueError(f"{what}: face_mask is on {mask.device}, vertices on {dev}")
        mask = mask.to(torch.uint8).contiguous()
    if uniforms is not None:
        if seed is not None:
            raise ValueError(f"{what}: give uniforms or seed, not both")
        u = _as_tensor(what, "uniforms", uniforms, dev)
        if tuple(u.shape) != (n, 3) or u.dtype != torch.float64:
            raise ValueError(f"{what}: uniforms must be float64 {(n, 3)}, got {tuple(u.shape)} {u.dtype}")
        if not _same_device(u.device, dev):
            raise ValueError(f"{what}: uniforms are on {u.device}, vertices on {dev}")
        u = u.contiguous()
    elif seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer))):
        raise ValueError(f"{what}: seed must be an integer, got {type(seed).__name__}")
    if out is not None:
        out = _check_out(what, out, n, dev)
    require_cuda(v, f, mask)
    if uniforms is None:
        gen = None
        if seed is not None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
        u = torch.rand((n, 3), dtype=torch.float64, device=dev, generator=gen)
    if out is None:
        out = SurfaceSamples.empty(n, dev)
    L = _lib.lib()
    nbytes = ctypes.c_int64()
    check(L.d3ga_surface_sample_scratch_bytes(F, ctypes.byref(nbytes)), "d3ga_surface_sample_scratch_bytes")
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    with torch.no_grad():
        check(L.d3ga_surface_sample(V, F, n, dptr(v), dptr(f), dptr(mask), dptr(u), dptr(out.points), dptr(out.rotations), dptr(out.faces),
                                    dptr(out.face_id), dptr(out.barys), dptr(scratch), nbytes.value, dptr(out.status), int(block),
                                    stream_handle()), "d3ga_surface_sample")
    return out


def _normals(what, vertices, faces, amount, want_normals):
    topo = faces if isinstance(faces, MeshTopology) else None
    v, f = _mesh(what, vertices, faces)
    amount = float(amount)
    if not math.isfinite(amount):
        raise ValueError(f"{what}: amount = {amount} is not finite")
    V, F, dev = v.shape[0], f.shape[0], v.device
    require_cuda(v, f)
    if topo is None:
        topo = MeshTopology(f)
    offsets, idx = topo.csr(V, dev)
    res = torch.empty_like(v)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.no_grad():
        check(_lib.lib().d3ga_vertex_normals_angle(V, F, dptr(v), dptr(f), dptr(offsets), dptr(idx), amount, dptr(res) if want_normals else None,
                                                   None if want_normals else dptr(res), dptr(status), stream_handle()),
              "d3ga_vertex_normals_angle")
    return res


def vertex_normals_angle(vertices, faces):
    """Angle-weighted vertex normals, trimesh's `mesh.vertex_normals` rule: n_v = normalize(sum over v's faces, ascending, of
    (the face's angle at v) x (its unit normal)); a vertex of no face, or of a zero sum, gets zero.  -> (V,3) float64.  The
    existing `vertex_normals` (pytorch3d's area-weighted rule) is something else and stays as it is.  faces: (F,3) or a
    MeshTopology (its vertex -> face lists are reused)."""
    return _normals("vertex_normals_angle", vertices, faces, 0.0, True)


def inflate(vertices, faces, amount):
    """vertices + amount x angle-weighted vertex normals (lib/cage.py:271-272) -> (V,3) float64, one launch."""
    return _normals("inflate", vertices, faces, amount, False)


def _get(cfg, key, default=None):
    if isinstance(cfg, dict) or hasattr(cfg, "keys"):
        return cfg[key] if key in cfg else default
    return getattr(cfg, key, default)


def _has(cfg, key):
    return key in cfg if (isinstance(cfg, dict) or hasattr(cfg, "keys")) else hasattr(cfg, key)


def _keys(cfg):
    return list(cfg.keys()) if (isinstance(cfg, dict) or hasattr(cfg, "keys")) else list(vars(cfg))


def body_surface_draws(face_to_label, cages, name, face_mask=None, neighbours=None):
    """The host logic of `CageBase.sample_body_surface` for cage `name` ("body" or "face"): the list of (mask (F,) bool, count)
    draws in the order the reference concatenates them -- `n_under_gaussians` over the whole body first (body cage of a
    multi-cage avatar only; without the face region when there is a face cage), then `n_gaussians` outside the garments
    (lib/cage.py:200-215: the face cage samples the face region, the body cage avoids it when a face cage exists).
    face_to_label (F,) integers; cages: the configuration's `cages` mapping (each entry with `label_id`, `n_gaussians`, ...);
    face_mask (F,) bool: the face region (`get_face_mask`), default none.  The reference also draws ring-intersection samples
    (`grow_mask_region` by 10 rings, `n_intsec_gaussians`) and discards them: they are not drawn, and `neighbours` -- the table
    they would need -- is accepted and not read."""
    what = "body_surface_draws"
    labels = face_to_label.detach().cpu().numpy() if torch.is_tensor(face_to_label) else np.asarray(face_to_label)
    if labels.ndim != 1 or labels.shape[0] < 1 or labels.dtype.kind not in "iu":
        raise ValueError(f"{what}: expected face_to_label (F,) of integers, got {tuple(labels.shape)} {labels.dtype}")
    F = labels.shape[0]
    keys = _keys(cages)
    if name not in ("body", "face") or name not in keys:
        raise ValueError(f"{what}: name must be 'body' or 'face' and one of the cages {keys}, got {name!r}")
    if face_mask is None:
        face = np.zeros(F, bool)
    else:
        face = face_mask.detach().cpu().numpy() if torch.is_tensor(face_mask) else np.asarray(face_mask)
        if face.shape != (F,) or face.dtype.kind not in "bu":
            raise ValueError(f"{what}: expected face_mask ({F},) bool, got {tuple(face.shape)} {face.dtype}")
        face = face.astype(bool)
    garment = np.zeros(F, bool)
    for key in keys:
        if key not in ("body", "face"):
            for label in _get(cages[key], "label_id", []) or []:
                if label != -1:
                    garment |= labels == label
    outside = ~garment
    if name == "face":
        outside = face.copy()
    if name == "body" and "face" in keys:
        outside = outside & ~face
    cfg = cages[name]
    if not _has(cfg, "n_gaussians") or int(_get(cfg, "n_gaussians")) < 1:
        raise ValueError(f"{what}: cage {name!r} needs n_gaussians >= 1")
    draws = []
    if len(keys) > 1 and name == "body" and _has(cfg, "n_under_gaussians"):
        count = int(_get(cfg, "n_under_gaussians"))
        if count < 1:
            raise ValueError(f"{what}: n_under_gaussians = {count}, expected at least 1")
        draws.append((~face if "face" in keys else np.ones(F, bool), count))
    draws.append((outside, int(_get(cfg, "n_gaussians"))))
    return draws


def sample_initial_points(vertices, faces, cage_config, config, face_to_label=None, *, face_mask=None, neighbours=None, uniforms=None,
                          seed=None):
    """`CageBase.sample_initial_points` -> (points (n,3) f32, rotations (n,4) f32 wxyz, faces (n,3) int32, barys (n,3) f32).

    cage_config: the cage's entry (`cage_name`, `n_gaussians`, `inflate`, optionally `n_under_gaussians`); config: the whole
    configuration (`config.cages`).  The body and face cages sample the body mesh through `body_surface_draws` (needs
    face_to_label); every other cage samples the mesh inflated along its angle-weighted vertex normals by `cage_config.inflate`,
    and its frames and barycentrics are those of the inflated mesh, as in the reference.  uniforms: (total,3) float64 for all
    draws in order, else drawn from `seed`.  Reads the status back once and raises ValueError if a draw had nothing to sample."""
    what = "sample_initial_points"
    name = _get(cage_config, "cage_name")
    if not isinstance(name, str):
        raise ValueError(f"{what}: cage_config.cage_name must be a string, got {name!r}")
    if name in ("body", "face"):
        if face_to_label is None:
            raise ValueError(f"{what}: the {name} cage needs face_to_label")
        cages = _get(config, "cages")
        if cages is None:
            raise ValueError(f"{what}: config has no cages")
        if name not in _keys(cages):
            cages = {**{k: cages[k] for k in _keys(cages)}, name: cage_config}
        draws = body_surface_draws(face_to_label, cages, name, face_mask, neighbours)
        verts = vertices
    else:
        if not _has(cage_config, "n_gaussians") or int(_get(cage_config, "n_gaussians")) < 1:
            raise ValueError(f"{what}: cage {name!r} needs n_gaussians >= 1")
        draws = [(None, int(_get(cage_config, "n_gaussians")))]
        verts = None
    total = sum(c for _, c in draws)
    v, f = _mesh(what, vertices, faces)
    if uniforms is not None:
        if not torch.is_tensor(uniforms) or tuple(uniforms.shape) != (total, 3) or uniforms.dtype != torch.float64:
            raise ValueError(f"{what}: uniforms must be a float64 tensor {(total, 3)}")
        if seed is not None:
            raise ValueError(f"{what}: give uniforms or seed, not both")
    for mask, _ in draws:
        if mask is not None and mask.shape[0] != f.shape[0]:
            raise ValueError(f"{what}: face_to_label has {mask.shape[0]} entries, the mesh {f.shape[0]} faces")
    require_cuda(v, f)
    if verts is None:
        v = inflate(v, f, float(_get(cage_config, "inflate", 0.0)))
    if uniforms is None:
        gen = None
        if seed is not None:
            gen = torch.Generator(device=v.device)
            gen.manual_seed(int(seed))
        uniforms = torch.rand((total, 3), dtype=torch.float64, device=v.device, generator=gen)
    out = SurfaceSamples.empty(total, v.device)
    a = 0
    for mask, count in draws:
        m = None if mask is None else torch.from_numpy(mask).to(v.device)
        sample_surface(v, f, count, face_mask=m, uniforms=uniforms[a:a + count], out=out.rows(a, a + count))
        a += count
    out.check()
    return out.points, out.rotations, out.faces, out.barys


def init_cage_parameters(points, rotations, n_color_features, max_sh_degree, use_shs=True, generator=None):
    """The parameter block of `CageNet.__init__` (models/cage_net.py:57-77) -> dict of float32 tensors under the reference's
    parameter names: colors_feat (P, n_color_features) = rand * 0.33, rotation (P,4), scaling (P,3) =
    log sqrt(clamp_min(knn_mean_dist2(points), 1e-7)) in every column (the existing kernel), and with use_shs: opacities (P,1) =
    inverse_sigmoid(0.2), features_dc (P,1,3) = rand / 255, features_rest (P, (max_sh_degree + 1)^2 - 1, 3) zeros.  generator: a
    torch.Generator on the points' device (colours are drawn first, then the SH base colours).  Wrap the values in nn.Parameter."""
    what = "init_cage_parameters"
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 4 or points.dtype != torch.float32:
        raise ValueError(f"{what}: expected points (P,3) float32 with P >= 4, got "
                         f"{(tuple(points.shape), points.dtype) if torch.is_tensor(points) else type(points).__name__}")
    P = points.shape[0]
    if not torch.is_tensor(rotations) or tuple(rotations.shape) != (P, 4) or rotations.dtype != torch.float32:
        raise ValueError(f"{what}: expected rotations {(P, 4)} float32")
    if rotations.device != points.device:
        raise ValueError(f"{what}: rotations are on {rotations.device}, points on {points.device}")
    n_color_features, max_sh_degree = int(n_color_features), int(max_sh_degree)
    if n_color_features < 1 or not 0 <= max_sh_degree <= 3:
        raise ValueError(f"{what}: n_color_features = {n_color_features} (>= 1), max_sh_degree = {max_sh_degree} (0 .. 3)")
    if generator is not None and (not isinstance(generator, torch.Generator) or not _same_device(generator.device, points.device)):
        raise ValueError(f"{what}: generator must be a torch.Generator on {points.device}")
    require_cuda(points, rotations)
    from .tetra import knn_mean_dist2
    dev = points.device
    with torch.no_grad():
        colors = torch.rand((P, n_color_features), dtype=torch.float32, device=dev, generator=generator) * 0.33
        shs = torch.rand((P, 3), dtype=torch.float32, device=dev, generator=generator) / 255
        dist2 = torch.clamp_min(knn_mean_dist2(points), 0.0000001)
        params = {"colors_feat": colors.contiguous(), "rotation": rotations.detach().clone().contiguous(),
                  "scaling": torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3).contiguous()}
        if use_shs:
            features = torch.zeros((P, 3, (max_sh_degree + 1) ** 2), dtype=torch.float32, device=dev)
            features[:, :3, 0] = shs
            x = 0.2 * torch.ones((P, 1), dtype=torch.float32, device=dev)
            params["opacities"] = torch.log(x / (1 - x)).contiguous()
            params["features_dc"] = features[:, :, 0:1].transpose(1, 2).contiguous()
            params["features_rest"] = features[:, :, 1:].transpose(1, 2).contiguous()
    return params
