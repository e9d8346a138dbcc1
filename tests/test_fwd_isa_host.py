"""Static checks on the compiled compositing forward (no GPU): every instantiation of composite_fwd_q_kernel is cross-compiled
to gfx950 assembly with build.py's flags and read with the parser of tools/isa_mix_fwd.py.

The blend loop's slab records are laid out so that every dword a read fetches is used: a read with a dead dword narrows to
ds_read_b96, which occupies the LDS array for 8 cycles against 4 for a ds_read_b128.  What is pinned here is that property, the
register / scratch / LDS budget that keeps five wavefronts per SIMD and twenty workgroups per CU, and the headline's LDS price.
"""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")

# ScratchSize (bytes per lane) of the commit before the slab layout changed, by (DUAL, DEPTH, L1V, PVB, WIN): a bound, not a target
PARENT_SCRATCH = {
    "00000": 0, "00001": 0, "00010": 0, "00011": 0, "00100": 0, "00101": 16, "00110": 0, "00111": 16,
    "01000": 0, "01001": 0, "01010": 0, "01011": 0, "01100": 16, "01101": 16, "01110": 16, "01111": 16,
    "10000": 56, "10001": 36, "10010": 56, "10011": 36, "11000": 60, "11001": 48, "11010": 60, "11011": 48,
}


@pytest.fixture(scope="module")
def analysis():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_mix_fwd
    return isa_mix_fwd, isa_mix_fwd.analyse()


def _key(flags):
    return "".join("1" if f else "0" for f in flags)


def test_every_instantiation_is_there(analysis):
    _, res = analysis
    assert sorted(_key(f) for f in res) == sorted(PARENT_SCRATCH)


def test_blend_loop_reads_no_dead_dwords(analysis):
    _, res = analysis
    for flags, a in res.items():
        lds = a["blend"]["lds"]
        assert "ds_read_b96" not in lds and "ds_read_u16" not in lds, (_key(flags), lds)
        assert "lds_unpriced" not in a["blend"], (_key(flags), a["blend"]["lds_unpriced"])
        assert a["blend"]["valu"]["trans"] == 2, (_key(flags), a["blend"]["valu"])      # the loop that was found is the blend loop


def test_budget_of_every_instantiation(analysis):
    _, res = analysis
    for flags, a in res.items():
        m = a["meta"]
        assert m["scratch"] <= PARENT_SCRATCH[_key(flags)], (_key(flags), m)
        assert m["occupancy"] == 5, (_key(flags), m)
        assert m["vgprs"] <= 96 and m["lds_bytes"] <= 7168, (_key(flags), m)


def test_headline_lds_price(analysis):
    tool, res = analysis
    a = res[tool.HEADLINE]
    print(a["meta"], a["blend"])
    assert a["blend"]["lds_array_cycles"] <= 24, a["blend"]
    assert a["meta"]["vgprs"] <= 96 and a["meta"]["lds_bytes"] <= 7168 and a["meta"]["scratch"] == 0, a["meta"]
