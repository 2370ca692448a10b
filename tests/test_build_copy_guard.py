"""Not-GPU guard on the BUILT library: the copy guard's kernels exist -- the scan and its init kernel (composer_amd/csrc/copyguard.hip)
and the history gather of the decode chains (decode.hip) --, one instantiation each, use no scratch and spill no register, read out of
the code-object metadata with tests/test_build_score.py's reader.  The scan's static LDS is what DESIGN section 4 states: the table
"last token of a window -> rows", 512 heads of 4 bytes and 256 links of 2 bytes; the windows themselves (B x M x 2 bytes, at most
32 KiB) are dynamic and not part of the figure.  None of the names contains `novelty_` (tests/test_build_novelty.py counts those)."""
import os
import re

from test_build_score import _kernel_notes

HERE = os.path.dirname(os.path.abspath(__file__))
SCAN_STATIC_LDS = 512 * 4 + 256 * 2


def test_copy_guard_kernels_exist_without_scratch_or_spills():
    notes = _kernel_notes()
    for name, lds in (("copyguard_scan_kernel", SCAN_STATIC_LDS), ("copyguard_init_kernel", 0), ("dec_guard_gather_kernel", 0)):
        found = {n: v for n, v in notes.items() if name in n}
        assert len(found) == 1, (name, sorted(found))
        (n, v), = found.items()
        assert "novelty_" not in n
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (name, v)
        assert v["lds"] == lds, (name, v)


def test_the_design_states_the_same_lds_figure():
    text = open(os.path.join(HERE, "..", "DESIGN.md")).read()
    m = re.search(r"copyguard_scan_kernel[^\n]*?(\d+) B of static LDS", text)
    assert m and int(m.group(1)) == SCAN_STATIC_LDS, m and m.group(0)


def test_the_library_binds_the_copy_guard():
    from composer_amd import _lib
    for name in ("cmp_decode_copy_guard", "cmp_decode_copy_guard_state", "cmp_k_copy_bans"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
