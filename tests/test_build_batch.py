"""Not-GPU guard on the BUILT library: batch_rows_kernel (composer_amd/csrc/batch.hip) exists, uses no scratch and spills no
register, read out of the code-object metadata the way tests/test_build_guards.py reads it (tests/test_build_score.py's reader).
Its only LDS are the per-wave totals of the three block scans."""
from test_build_score import _kernel_notes


def test_batch_rows_kernel_exists_without_scratch_or_spills():
    ks = {n: v for n, v in _kernel_notes().items() if "batch_rows_kernel" in n}
    assert len(ks) == 1, sorted(ks)
    v = next(iter(ks.values()))
    assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, ks
    assert 0 < v["lds"] <= 256, ks             # 4 waves x (two 64-bit totals + one count)
