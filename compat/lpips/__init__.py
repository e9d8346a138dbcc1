"""Drop-in `lpips` package surface (recorder/heatmap.py:9, 13 does `import lpips; lpips.LPIPS("vgg").cuda()`): the HIP metric of
d3ga_amd/lpips.py.  Weights come from the caller or from the path in D3GA_LPIPS_WEIGHTS; nothing is ever fetched."""
from d3ga_amd.lpips import LPIPS  # noqa: F401

__all__ = ["LPIPS"]
