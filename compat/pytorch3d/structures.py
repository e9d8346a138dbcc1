"""pytorch3d.structures.Meshes / Pointclouds for padded tensors, as the reference builds them (recorder/mesh_renderer.py:61,70,
lib/segmentation.py:56, recorder/pc_renderer.py:65).  Lists of tensors and heterogeneous batches are not built."""
import torch

__all__ = ["Meshes", "Pointclouds"]

_topology_cache = []            # [(faces tensor, its version, MeshTopology)]: the reference passes the same faces every frame


def _shared_topology(faces):
    """The MeshTopology of a padded faces tensor (M,F,3), cached on the tensor and its version counter.  Building it reads
    the faces on the host (the one synchronisation, once per tensor); M > 1 face lists are compared there as well."""
    from d3ga_amd.mesh_render import MeshTopology
    for t, version, topo in _topology_cache:
        if t is faces and version == faces._version:
            return topo
    host = faces.detach().cpu()
    if host.shape[0] > 1 and not bool((host == host[:1]).all()):
        raise NotImplementedError("Meshes: faces with different face lists per mesh (a heterogeneous batch) are not built")
    topo = MeshTopology(host[0].numpy())
    del _topology_cache[:]
    _topology_cache.append((faces, faces._version, topo))
    return topo


class Meshes:
    """Meshes(verts (N,V,3), faces (M,F,3) int32 or int64 with M in {1, N}, textures=None).  With M = N > 1 all face lists must
    be equal.  `faces_packed()` offsets mesh n by n V; `verts_normals_packed()` is d3ga_amd's `vertex_normals` (GPU)."""

    def __init__(self, verts=None, faces=None, textures=None, *, verts_normals=None):
        if verts_normals is not None:
            raise NotImplementedError("Meshes: verts_normals is not built")
        if not torch.is_tensor(verts) or not torch.is_tensor(faces):
            raise NotImplementedError("Meshes: verts and faces as lists of tensors are not built; pass padded tensors")
        if verts.dim() != 3 or verts.shape[-1] != 3:
            raise ValueError(f"Meshes: expected verts (N,V,3), got {tuple(verts.shape)}")
        if faces.dim() != 3 or faces.shape[-1] != 3:
            raise ValueError(f"Meshes: expected faces (M,F,3), got {tuple(faces.shape)}")
        if faces.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"Meshes: faces must be int32 or int64, got {faces.dtype}")
        if faces.shape[0] not in (1, verts.shape[0]):
            raise ValueError(f"Meshes: {verts.shape[0]} meshes but {faces.shape[0]} face lists")
        self._verts, self._faces, self.textures = verts, faces, textures
        self.device = verts.device
        self._topo = None

    def __len__(self):
        return self._verts.shape[0]

    def topology(self):
        if self._topo is None:
            self._topo = _shared_topology(self._faces)
        return self._topo

    def verts_padded(self):
        return self._verts

    def verts_packed(self):
        return self._verts.reshape(-1, 3)

    def faces_padded(self):
        return self._faces.expand(len(self), -1, -1).long()

    def faces_packed(self):
        N, V = self._verts.shape[0], self._verts.shape[1]
        offset = torch.arange(N, device=self._faces.device, dtype=torch.int64)[:, None, None] * V
        return (self._faces.long().expand(N, -1, -1) + offset).reshape(-1, 3)

    def verts_normals_padded(self):
        from d3ga_amd.mesh_render import vertex_normals
        return vertex_normals(self._verts.detach().float(), self.topology())

    def verts_normals_packed(self):
        return self.verts_normals_padded().reshape(-1, 3)


class Pointclouds:
    """Pointclouds(points (N,P,3), features (N,P,C) or (1,P,C) or None)."""

    def __init__(self, points, normals=None, features=None):
        if normals is not None:
            raise NotImplementedError("Pointclouds: normals is not built")
        if not torch.is_tensor(points) or (features is not None and not torch.is_tensor(features)):
            raise NotImplementedError("Pointclouds: points and features as lists of tensors are not built; pass padded tensors")
        if points.dim() != 3 or points.shape[-1] != 3:
            raise ValueError(f"Pointclouds: expected points (N,P,3), got {tuple(points.shape)}")
        if features is not None and (features.dim() != 3 or features.shape[1] != points.shape[1] or
                                     features.shape[0] not in (1, points.shape[0])):
            raise ValueError(f"Pointclouds: expected features (N,P,C), got {tuple(features.shape)}")
        self._points, self._features = points, features
        self.device = points.device

    def __len__(self):
        return self._points.shape[0]

    def points_padded(self):
        return self._points

    def points_packed(self):
        return self._points.reshape(-1, 3)

    def features_padded(self):
        return self._features

    def features_packed(self):
        return None if self._features is None else self._features.expand(len(self), -1, -1).reshape(-1, self._features.shape[-1])
