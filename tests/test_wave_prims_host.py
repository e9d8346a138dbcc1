"""csrc/wave_prims.h is the one place for the 64-lane butterfly sum and the two-level scan; csrc/d3ga_internal.h the one place
for the once-per-device guard.  Read from the sources, as test_losses_host.py reads its constants: a private copy in a new
.hip file fails here, before anyone has to review it."""
import os
import re

from d3ga_amd.csrc import build

CSRC = os.path.dirname(os.path.abspath(build.__file__))
# Names that contain "wave_sum" and are something else: deform.hip's DPP sum (another instruction sequence on purpose) and
# the host mirror of the butterfly on an array, which the g++ build of objective_math.h runs.
OTHER_SUMS = {"wave_sum_", "obj_wave_sum"}
BUTTERFLY = re.compile(r"\bv \+= __shfl_xor\(v, off")
# the same loop under another variable's name (a sum over part of a wavefront, off < G, is no copy)
RENAMED = re.compile(r"for \(int off = \w+( / 2)?; off (>= 1|> 0); off >>= 1\)\s*\{?\s*(\w+) \+= __shfl_xor\(\3, off")
DEFINED = re.compile(r"^[\w \t]*\b(?:float|double|T)\s+(\w*wave_sum\w*)\s*\(", re.M)


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "wave_prims.h":
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read()


def test_the_header_is_a_build_dependency():
    assert "wave_prims.h" in build.HEADERS
    assert os.path.exists(os.path.join(CSRC, "wave_prims.h"))


def test_no_private_copy_of_the_wavefront_sum():
    for name, src in _sources():
        assert not BUTTERFLY.search(src), name
        if name != "raster_composite.hip":                 # its backward's sum over `d`: device code this header was not to touch
            assert not RENAMED.search(src), name
        assert set(DEFINED.findall(src)) <= OTHER_SUMS, (name, DEFINED.findall(src))


def test_the_patterns_find_the_copies_they_are_for():
    """The shapes the copies had, and the header's own."""
    with open(os.path.join(CSRC, "wave_prims.h")) as f:
        src = f.read()
    assert BUTTERFLY.search(src) and DEFINED.findall(src) == ["wave_sum"]
    assert DEFINED.findall("__device__ __forceinline__ float calib_wave_sum(float v) {") == ["calib_wave_sum"]
    assert RENAMED.search("#pragma unroll\n    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);")
    assert RENAMED.search("for (int off = kObjLanes / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);")
    assert RENAMED.search("for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);")
    assert not RENAMED.search("for (int off = 1; off < G; off <<= 1) d += __shfl_xor(d, off);")      # a sub-group sum is no copy


def test_no_unsynchronised_per_device_flag():
    for name, src in _sources():
        assert "static bool attr[" not in src, name
