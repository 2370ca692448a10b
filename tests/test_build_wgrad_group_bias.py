"""Not-GPU guard on the BUILT library: the grouped weight-gradient kernels -- the float-atomic form, whose stage loop now has a
second instantiation with the four column-sum MFMAs, and the last-arriver form -- must hold their accumulators, fragments and the
column sums in registers: scratch bytes and spilled registers read from the code-object metadata (the helper of
tests/test_build_guards.py) are zero.

Both were at the 256-register limit with a handful of spilled registers before (the float-atomic form 24 bytes / 5 registers, the
last-arriver form 204 / 54): per-lane addresses of cold per-item code -- the epilogues' column / row offsets, the item scheduler's
counter addresses -- hoisted out of the item loop and kept live across the k-loops, and sixteen 16-byte loads in flight in the
last-arriver reduction.  gemm.hip computes those addresses where they are used (p4_body: cold_lane) and keeps eight loads in flight."""
import pytest

from test_build_guards import _demangle, _kernels


@pytest.mark.parametrize("kernel", ["gemm_wgrad_group_kernel", "gemm_wgrad_group_la_kernel"])
def test_grouped_wgrad_kernels_use_no_scratch(kernel):
    ks = _kernels()
    pretty = _demangle(list(ks))
    mine = {pretty.get(n, n): v for n, v in ks.items() if kernel + "(" in pretty.get(n, n)}
    assert len(mine) == 1, sorted(mine)
    (name, v), = mine.items()
    print("%s: scratch %d bytes, %d spilled registers, %d VGPRs" % (kernel, v["scratch"], v["spill"], v["vgpr"]))
    assert v["scratch"] == 0 and v["spill"] == 0, (name, v)
