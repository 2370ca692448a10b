"""Not-GPU guards on the BUILT library's device code: the hot kernels must not spill.

Round 5 found two ways a spill turns into a large slowdown that no parity test sees (profiles/NEGATIVE_RESULTS.md, round 5): the
persistent 256x256 GEMM sits at the 256-register limit, and a few more live registers in an epilogue kind made hipcc (a) spill the
address registers of the next k-slab's LDS-DMA and reload them between the DMA pieces behind `s_waitcnt vmcnt(0)`, or (b) put a
full `s_waitcnt vmcnt(0)` at the top of the k-step.  The code-object metadata of every kernel (scratch bytes, spilled registers)
is read back out of libcomposer_hip.so here, so such a build fails the CPU suite before it reaches the GPU.
"""
import os
import re
import subprocess
import tempfile

import pytest

from composer_amd import _lib

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _kernels():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(LLVM + "/clang-offload-bundler")):
        pytest.skip("library or LLVM tools missing")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, _lib.LIB_PATH], check=True)
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
            for blk in notes.split(".name:")[1:]:
                name = blk.split()[0]
                g = lambda k: int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1))
                try:
                    out[name] = {"scratch": g(".private_segment_fixed_size"), "spill": g(".vgpr_spill_count"), "vgpr": g(".vgpr_count")}
                except AttributeError:
                    pass
    return out


def _demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.split("\n")))


def test_hot_kernels_do_not_spill():
    ks = _kernels()
    assert len(ks) > 50, len(ks)
    pretty = _demangle(list(ks))
    hot = {}
    for n, v in ks.items():
        p = pretty.get(n, n)
        # every compile-time epilogue kind of the forward / dgrad layout of the persistent 256x256 kernel (EPI_GENERIC = 0 is the
        # run-time fallback, not on the benchmark path), the grouped weight-gradient kernel, the bf16 attention kernels
        m = re.match(r"void gemm_bf16_256_kernel<true, true, true, (\d+)", p)
        # (c++filt leaves the __bf16 instantiations of the attention kernels mangled: `DF16b`; the forward's mask-term variants --
        # an inspection path, second bool -- are not hot)
        if ((m and int(m.group(1)) != 0) or "gemm_wgrad_group_kernel" in p or re.search(r"attn_(dq|dkv)_kernelIDF16bLi64E", n)
                or re.search(r"attn_fwd_kernelIDF16bLi64ELb[01]ELb0ELb0E", n)):
            hot[p] = v
    assert len(hot) >= 18 and sum("attn_" in p for p in hot) == 6, sorted(hot)
    # The GEMM kinds: no scratch at all.  The grouped weight-gradient kernel and the attention kernels have carried a handful of
    # spilled registers since round 3, every one stored / reloaded in set-up or tear-down blocks that hold no MFMA (checked in the
    # -save-temps assembly); the bound keeps them from growing into the loops unnoticed.
    bad = {}
    for p, v in hot.items():
        limit = 0 if "gemm_bf16_256_kernel" in p else (5 if "wgrad_group" in p else 11)
        if v["spill"] > limit or v["scratch"] > 8 * limit:
            bad[p] = v
    assert not bad, bad
    # round 5's small-grid kernels (the reference's default configuration): the key-split attention kernels at head size 16 and the
    # four-stage ring kinds of the 128x128 GEMM kernel count their LDS-DMA / staging waits by hand -- no scratch traffic inside them
    small = {p: v for p, v in ((pretty.get(n, n), v) for n, v in ks.items())
             if re.search(r"attn_(bwd_ks|dq_ks|dkv_ks)_kernelIDF16bLi16E", p) or re.search(r"attn_fwd_kernelIDF16bLi16ELb[01]ELb0ELb1E", p)
             or re.match(r"void gemm_bf16_fast_kernel<true, true, true, [1-4], true>", p)}
    assert len(small) == 12, sorted(small)
    assert not {p: v for p, v in small.items() if v["spill"] or v["scratch"]}, small


def test_shipped_translation_units_hold_shipped_kernels_only():
    """Every kernel lives in the tree once.  The sources the product library is built from carry no measurement-only branch (no
    `COMPOSER_EXPERIMENTS`, no `*_DIAG` ladder; running tools/strip_lab.py over them again changes nothing), and every `*.hip` under
    composer_amd/csrc/, at any depth, is one of them: no kernel source can sit in the tree without being shipped.  The measurement builds,
    the round-3 attention forwards and the first-generation decode kernels are in history: `git show a635116:composer_amd/csrc/experiments/<name>_lab.hip`."""
    import importlib.util
    import re as _re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("strip_lab", os.path.join(root, "tools", "strip_lab.py"))
    sl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sl)
    from composer_amd import build as B
    for src in B.SOURCES:
        text = open(os.path.join(B.CSRC, src)).read()
        assert not _re.search(r"COMPOSER_EXPERIMENTS|\b[A-Z0-9]+_DIAG\b", text), src
        assert sl.strip(text) == text, src
    assert all(os.path.dirname(s) == "" for s in B.SOURCES)                       # the library is built from csrc/ itself only
    found = []
    for d, subdirs, files in os.walk(B.CSRC):
        subdirs[:] = [s for s in subdirs if not (d == B.CSRC and s == "_obj")]      # the object cache is no source
        found += [os.path.relpath(os.path.join(d, f), B.CSRC) for f in files if f.endswith(".hip")]
    assert sorted(found) == sorted(B.SOURCES)                                     # every kernel source in the tree is shipped
    assert not os.path.exists(os.path.join(B.CSRC, "experiments"))
