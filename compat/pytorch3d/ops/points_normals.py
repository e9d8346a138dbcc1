"""pytorch3d.ops.points_normals: the reference imports `estimate_pointcloud_normals` (utils/graphics_utils.py:13) for
`get_normals`, which nothing calls."""

__all__ = ["estimate_pointcloud_normals"]


def estimate_pointcloud_normals(pointclouds, neighborhood_size=50, disambiguate_directions=True, *, use_symeig_workaround=True):
    raise NotImplementedError("pytorch3d.ops.points_normals.estimate_pointcloud_normals is not built: the reference's only use, "
                              "utils/graphics_utils.get_normals, has no caller")
