"""CPU: the comparison the device test of the novelty kernel uses (tests/novelty_cases.py: compare, the poison the outputs are pre-filled
with) must reject a wrong kernel.  Seven fake kernels, each wrong in one way the real one (composer_amd/csrc/novelty.hip) could be,
run on the cases' inputs; each has to fail the comparison on at least one case, and the faithful fake has to pass on all of them."""
import numpy as np
import pytest

import novelty_cases as nc
from composer_amd import novelty

FLAWS = ("ignores_piece_starts", "clips_the_transposition", "ties_to_the_highest_p", "drops_the_last_diagonal_of_a_block",
         "forgets_the_carry_between_s_chunks", "off_by_one_at_min_match", "leaves_the_padded_tail_unwritten")
CASES = ("n256", "n257b", "n5000_fold", "n5000_long")           # small enough to run eight fakes each; between them they hold every feature


def clipped_query(x, k, layout, velocity):
    v0, vn = velocity
    x = np.where((x >= v0) & (x < v0 + vn), v0, x)
    out = x.copy()
    for base in (layout.note_on0, layout.note_off0):
        note = (x >= base) & (x < base + 128)
        out[note] = base + np.clip(x[note] - base + k, 0, 127)
    return out


def fake_kernel(name, flaw=None):
    """What a kernel with one flaw writes into outputs pre-filled the way the device test pre-fills them."""
    c = nc.case(name)
    n, ld = c.n, c.ld
    vel = c.velocity or (0, 0)
    out_len = np.full((c.B, ld), -1, np.int32)
    out_pos = np.full((c.B, ld), nc.POISON_POS, np.int64)
    out_k = np.full((c.B, ld), nc.POISON_K, np.int32)
    cf = np.where((c.corpus.astype(np.int64) >= vel[0]) & (c.corpus < vel[0] + vel[1]), vel[0], c.corpus).astype(np.int32)
    go_on = np.ones(n, np.int32)
    go_on[n - 1] = 0
    if flaw != "ignores_piece_starts":
        go_on[c.starts[c.starts >= 1] - 1] = 0
    p_idx = np.arange(n)
    for b, row in enumerate(c.rows):
        L = len(row)
        x = row.astype(np.int64)
        best_len, best_pos, best_k = np.zeros(L, np.int32), np.full(L, -1, np.int64), np.zeros(L, np.int32)
        for k in novelty.rank_order(c.N):
            xk = (clipped_query if flaw == "clips_the_transposition" and k else novelty.map_query)(x, k, c.layout, vel)
            prev = np.zeros(n + 1, np.int32)
            for s in range(L - 1, -1, -1):
                if flaw == "forgets_the_carry_between_s_chunks" and (s + 1) % nc.KERNEL_SCHUNK == 0:
                    prev[:] = 0
                cur = (prev[1:] * go_on + 1) * (cf == xk[s])
                if flaw == "drops_the_last_diagonal_of_a_block":
                    cur[(p_idx - s + ld - 1) % nc.KERNEL_BLOCK == nc.KERNEL_BLOCK - 1] = 0
                m = int(cur.max())
                if m > best_len[s]:
                    p = n - 1 - int(cur[::-1].argmax()) if flaw == "ties_to_the_highest_p" else int(cur.argmax())
                    best_len[s], best_pos[s], best_k[s] = m, p, k
                prev[:n] = cur
        low = best_len <= c.min_match if flaw == "off_by_one_at_min_match" else best_len < c.min_match
        best_len[low], best_pos[low], best_k[low] = 0, -1, 0
        out_len[b, :L], out_pos[b, :L], out_k[b, :L] = best_len, best_pos, best_k
        if flaw != "leaves_the_padded_tail_unwritten":
            out_len[b, L:], out_pos[b, L:], out_k[b, L:] = 0, -1, 0
    return out_len, out_pos, out_k


def rejected(name, flaw):
    try:
        nc.compare(name, *fake_kernel(name, flaw))
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", CASES)
def test_the_faithful_fake_passes(name):
    nc.compare(name, *fake_kernel(name))


@pytest.mark.parametrize("flaw", FLAWS)
def test_a_wrong_kernel_is_rejected(flaw):
    caught = [name for name in CASES if rejected(name, flaw)]
    assert caught, "no case rejects a kernel that " + flaw.replace("_", " ")
