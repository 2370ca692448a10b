"""Not-GPU guard on the BUILT library: the novelty kernels (composer_amd/csrc/novelty.hip) exist -- one matching kernel per counter
count, one unpacking kernel --, use no scratch and spill no register, read out of the code-object metadata the way
tests/test_build_guards.py reads it (tests/test_build_score.py's reader).  The matching kernels' LDS is the staged corpus window
(256 + 512 codes) and the mapped query chunk (512 positions x 1 or 8 tokens), 4 bytes each; the unpacking kernel has none."""
from test_build_score import _kernel_notes


def test_novelty_kernels_exist_without_scratch_or_spills():
    ks = {n: v for n, v in _kernel_notes().items() if "novelty_" in n}
    match = {n: v for n, v in ks.items() if "novelty_match_kernel" in n}
    unpack = {n: v for n, v in ks.items() if "novelty_unpack_kernel" in n}
    assert len(match) == 2 and len(unpack) == 1 and len(ks) == 3, sorted(ks)
    # no kernel touches scratch memory or spills a vector register.  The matching kernels' staging code keeps the grid-stride,
    # row and chunk loops' scalars live and hipcc parks some of them in lanes of a vector register (6 and 36 at the time of
    # writing, none inside the loop over query positions): registers only, which `scratch == 0` holds; the unpacking kernel parks none.
    for n, v in ks.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, ks
        assert v["sgpr_spill"] == 0 or n in match, ks
    assert sorted(v["lds"] for v in match.values()) == [(256 + 512 + 512) * 4, (256 + 512 + 8 * 512) * 4], match
    assert all(v["lds"] == 0 for v in unpack.values()), unpack
