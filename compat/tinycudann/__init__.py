"""Drop-in `tinycudann` package surface for what the reference uses of it (models/mlp.py:13,166-179: `import tinycudann as
tcnn`, one `tcnn.Encoding` -- the degree-4 spherical-harmonics direction encoding): the HIP kernels behind
`d3ga_amd.mlp.sh4_direction_encoding`.  tiny-cuda-nn is CUDA only; every other configuration raises NotImplementedError.

One departure: tiny-cuda-nn returns half precision by default, this returns float32 (`dtype`, if given, must be float32)."""
import torch
from torch import nn

__all__ = ["Encoding"]


def _is_sh4(cfg, n_dims):
    """{"otype": "SphericalHarmonics", "degree": 4} over exactly three dimensions"""
    return (isinstance(cfg, dict) and cfg.get("otype") == "SphericalHarmonics" and cfg.get("degree") == 4 and
            cfg.get("n_dims_to_encode", n_dims) == 3 and n_dims == 3 and set(cfg) <= {"otype", "degree", "n_dims_to_encode"})


def _supported(cfg, n_dims):
    if _is_sh4(cfg, n_dims):
        return True
    # the Composite of it with a trailing Identity over the zero dimensions that remain, as models/mlp.py:166-179 writes it
    if isinstance(cfg, dict) and cfg.get("otype") == "Composite" and set(cfg) <= {"otype", "nested"}:
        nested = cfg.get("nested")
        return (isinstance(nested, (list, tuple)) and len(nested) in (1, 2) and _is_sh4(nested[0], n_dims) and
                all(isinstance(c, dict) and c.get("otype") == "Identity" and c.get("n_dims_to_encode", 0) == 0 and
                    set(c) <= {"otype", "n_dims_to_encode"} for c in nested[1:]))
    return False


class Encoding(nn.Module):
    """tcnn.Encoding(n_input_dims=3, encoding_config=...) for the degree-4 SphericalHarmonics encoding: forward(x (P,3)) ->
    (P,16) float32, differentiable as `sh4_direction_encoding` is.  Parameter-free."""

    def __init__(self, n_input_dims, encoding_config, dtype=None, seed=1337):
        super().__init__()
        if not _supported(encoding_config, n_input_dims):
            raise NotImplementedError(f"tinycudann.Encoding: encoding_config = {encoding_config!r} over n_input_dims = {n_input_dims!r}; only "
                                      "the degree-4 SphericalHarmonics encoding of 3 dimensions (alone or in a Composite with a trailing "
                                      "Identity) is built")
        if dtype not in (None, torch.float32):
            raise NotImplementedError(f"tinycudann.Encoding: dtype = {dtype!r}; the encoding returns float32")
        self.n_input_dims = 3
        self.n_output_dims = 16
        self.encoding_config = encoding_config
        self.dtype = torch.float32

    def forward(self, x):
        from d3ga_amd.mlp import sh4_direction_encoding
        return sh4_direction_encoding(x)
