"""pytorch3d.common: `compat.meshgrid_ij` (recorder/pc_renderer.py:19)."""
from . import compat  # noqa: F401
