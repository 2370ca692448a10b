"""Not-GPU guard on the built library: the batched decode kernels (decode_batch.hip) are in libcomposer_hip.so and run without
scratch -- no register spill on the per-token chain of cmp_decode_batch_steps."""
from test_build_guards import _demangle, _kernels


def test_batched_decode_kernels_exist_without_scratch():
    ks = _kernels()
    pretty = _demangle(list(ks))
    names = {pretty.get(n, n): v for n, v in ks.items()}
    want = ("decb_proj_kernel", "decb_attn_kernel", "decb_sample_kernel", "sample_rows_kernel", "decb_cache_fill_kernel")
    found = {w: [p for p in names if w in p] for w in want}
    assert all(found.values()), found
    assert len(found["decb_proj_kernel"]) == 6 and len(found["decb_attn_kernel"]) == 4, found
    bad = {p: v for w in want for p in found[w] for v in [names[p]] if v["scratch"] or v["spill"]}
    assert not bad, bad
