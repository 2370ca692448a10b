"""Not-GPU guard on the BUILT library: the kernels of the validation pass (composer_amd/csrc/evalpass.hip) use 0 bytes of scratch and
spill no register, read out of the code-object metadata the way tests/test_build_score.py reads it.  (The per-class sums live in
lanes, not in a register array indexed at run time, and the class ranges are found by a wave vote: either would show up here.)"""
import os
import re
import subprocess
import tempfile

import pytest

from composer_amd import _lib

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _kernel_notes():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(LLVM + "/clang-offload-bundler")):
        pytest.skip("library or LLVM tools missing")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        # (an explicit output file: with the input alone llvm-objcopy rewrites the library in place)
        subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, _lib.LIB_PATH, os.path.join(d, "copy.so")],
                       check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, s in enumerate(starts):                                   # one bundle per translation unit
            part = os.path.join(d, "b%d.bin" % i)
            open(part, "wb").write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            co = os.path.join(d, "b%d.co" % i)
            r = subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part,
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:                # one entry per kernel, opened by its first key
                g = lambda k: int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1))
                try:
                    name = re.findall(r"^\s+\.name:\s+(\S+)", blk, flags=re.M)[-1]
                    out[name] = {"scratch": g(".private_segment_fixed_size"), "vgpr_spill": g(".vgpr_spill_count"),
                                 "sgpr_spill": g(".sgpr_spill_count")}
                except (AttributeError, IndexError):
                    pass
    return out


def test_evalpass_kernels_use_no_scratch_and_no_spills():
    ks = {n: v for n, v in _kernel_notes().items() if "eval_rows_kernel" in n or "eval_fold_kernel" in n or "eval_windows_kernel" in n}
    # the row reduction in its three forms (16-byte loads, 4-byte loads, two passes over a wide row), the fold and the window cut
    assert len(ks) == 5 and sum("eval_rows_kernel" in n for n in ks) == 3, sorted(ks)
    assert all(v == {"scratch": 0, "vgpr_spill": 0, "sgpr_spill": 0} for v in ks.values()), ks
