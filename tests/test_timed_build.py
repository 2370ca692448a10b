"""Not-GPU guard on the built library: the three kernels that draw an id carry the budget's terms (phase, allowed TIME_SHIFT ids,
the polyphony bit) as a few uniform words -- none of them may have turned into scratch memory or a spilled vector register, or a scalar
register spilled into a vector lane."""
import os
import re
import subprocess
import tempfile

from test_build_guards import LLVM, MAGIC, _demangle, _kernels

DRAWING = ("dec_sample2_kernel", "decb_sample_kernel", "dec_slide_sample_kernel")


def _sgpr_spills():
    """{kernel: .sgpr_spill_count} of every kernel in the library (test_build_guards._kernels reads the vector counts only)"""
    from composer_amd import _lib
    out = {}
    with tempfile.TemporaryDirectory() as d:
        lib = os.path.join(d, "lib.so")                                    # (a copy: llvm-objcopy rewrites its input)
        open(lib, "wb").write(open(_lib.LIB_PATH, "rb").read())
        fat = os.path.join(d, "fat.bin")
        subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, s in enumerate(starts):
            part, co = os.path.join(d, "b%d.bin" % i), os.path.join(d, "b%d.co" % i)
            open(part, "wb").write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part,
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], capture_output=True)
            if not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for blk in notes.split(".name:")[1:]:
                m = re.search(r"\.sgpr_spill_count:\s+(\d+)", blk)
                if m:
                    out[blk.split()[0]] = int(m.group(1))
    return out


def test_the_kernels_that_draw_have_no_scratch_and_no_spill():
    from composer_amd import _lib
    assert "cmp_decode_budget" in _lib.SIGNATURES and "cmp_decode_budget_state" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "cmp_decode_budget"), "the library under test has no budget: nothing to guard"
    ks = _kernels()
    sg = _sgpr_spills()
    pretty = _demangle(list(ks))
    for name in DRAWING:
        found = {n: v for n, v in ks.items() if pretty.get(n, n).startswith(name + "(")}
        assert len(found) == 1, (name, sorted(found))
        (n, v), = found.items()
        assert v["scratch"] == 0 and v["spill"] == 0, (name, v)
        assert n in sg, (name, "no .sgpr_spill_count in the metadata")
        print(name, v, "sgpr spills", sg[n])
        # scalar registers spilled into vector lanes: none, as in the build of the commit before the budget (the batch-1 kernel
        # sits at the scalar register limit: two more words loaded in front of the draw were enough to make it spill)
        assert sg[n] == 0, (name, sg[n])
