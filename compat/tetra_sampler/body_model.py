"""`from tetra_sampler.body_model import SMPLlayer` (lib/smplman.py:9): the SMPL-X / SMPL body model of d3ga_amd
(HIP forward and backward).  It needs the licensed model files at `config.data.smplx_model`; without them construction
raises an error that is both FileNotFoundError and NotImplementedError."""
from d3ga_amd.body_model import SMPLlayer  # noqa: F401

__all__ = ["SMPLlayer"]
