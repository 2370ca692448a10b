"""Guard-banded operand arena and the per-element error bounds (GEMM, Adam) of the kernel-level tests.

Arena: ONE uint8 allocation (device or CPU) per test case, filled with byte 0xFF -- a NaN in bf16 and fp32, -1 in int32.  Every
operand of a launch is a window carved out of it: 256-byte aligned start, the end flush (no rounding up) against at least 4 KiB
of untouched 0xFF, a guard in front of the first window as well.  A window is [rows, ld]; the logical [rows, width] part holds
the data, the in-row padding width..ld holds `pad` (NaN unless the header states a zero-padding contract).  After the launch
`check()` proves that no guard byte and no padding byte of an output changed, that no input changed, and that a fully written
output holds no leftover 0xFF pattern and no non-finite value: a store outside the window, a load of padding or of a neighbour
that reaches a stored value (NaN propagates), and an element that was never written all fail it.

Bound: `gemm_bound` is the accumulation term  min(8 * q_seq, (K + 8) * 2^-24) * S  with S = |A|.|B| (+ |bias| ...) in float64 and
q_seq the error of a strictly sequential fp32 dot product of the same operands, measured on the CPU (`seq_fp32_matmul`);
`assert_within` applies it per element, with 2^-8 |ref| on top for a bf16 output.

Adam: `adam_reference` (float64), `adam_bounds` (per-element limits for p, m, v from one-ulp fp32 primitives), `adam_inputs` (one vector
in segments that put eps, the first step, pure decay and large gradients in view) and `adam_check` (all of it on one launch's results).
The same reference and bound hold a model's train step per element, fed with the gradient the device itself consumed.
"""
import numpy as np
import torch

GUARD = 4096
ALIGN = 256
EPS24 = 2.0 ** -24
BF16_OUT = 2.0 ** -8          # twice the half-ulp of round-to-nearest bf16: an epilogue may round once in fp32 before the store
SEQ_MARGIN = 8.0


class Slot:
    def __init__(self, arena, name, kind, dtype, rows, width, ld, start, pad_zero):
        self.arena, self.name, self.kind, self.dtype = arena, name, kind, dtype
        self.rows, self.width, self.ld, self.start, self.pad_zero = rows, width, ld, start, pad_zero
        self.esize = torch.empty(0, dtype=dtype).element_size()
        self.nbytes = rows * ld * self.esize
        self.t = arena.buf[start:start + self.nbytes].view(dtype).view(rows, ld)        # the whole window

    @property
    def logical(self):
        return self.t[:, :self.width]

    @property
    def vec(self):
        """The logical part of a one-row window as a 1-D tensor."""
        assert self.rows == 1
        return self.t[0, :self.width]

    def ptr(self):
        return self.t.data_ptr()

    def mem(self):
        """Flat typed view from the window's first element to the end of the arena: what a kernel's pointer can reach (the CPU
        fake kernels index it like device code does)."""
        n = (self.arena.buf.numel() - self.start) // self.esize * self.esize
        return self.arena.buf[self.start:self.start + n].view(self.dtype)

    def host(self):
        """The logical part as it is now, on the CPU."""
        return self.logical.detach().cpu().clone()


class Arena:
    def __init__(self, device="cuda", nbytes=8 << 20, big=False):
        assert nbytes <= (256 << 20 if big else 64 << 20), "an arena is at most 64 MB (256 MB for a case that says it is big)"
        self.device = device
        self.buf = torch.full((nbytes + ALIGN,), 0xFF, dtype=torch.uint8, device=device)
        self.base = (-self.buf.data_ptr()) % ALIGN          # buf[base] is 256-byte aligned
        self.cursor = self.base                              # end of the last window
        self.slots = []

    # ------------------------------------------------------------------ carving
    def _carve(self, name, kind, dtype, rows, width, ld, pad_zero=False):
        assert rows >= 1 and 1 <= width <= ld
        start = self.base + -(-(self.cursor - self.base + GUARD) // ALIGN) * ALIGN
        esize = torch.empty(0, dtype=dtype).element_size()
        assert start + rows * ld * esize + GUARD <= self.buf.numel(), "arena too small for %s" % name
        s = Slot(self, name or "%s%d" % (kind, len(self.slots)), kind, dtype, rows, width, ld, start, pad_zero)
        assert s.ptr() % ALIGN == 0
        self.cursor = start + s.nbytes
        self.slots.append(s)
        return s

    def _fill(self, s, host, pad):
        host = torch.as_tensor(host).reshape(s.rows, s.width)
        s.logical.copy_(host.to(s.dtype))
        if s.ld > s.width and pad is not None:
            s.t[:, s.width:] = pad
        return s

    def operand(self, host, dtype, rows, width, ld, pad=float("nan"), name=None):
        """An input.  Integer operands keep 0xFF (-1) as padding."""
        s = self._carve(name, "in", dtype, rows, width, ld)
        return self._fill(s, host, pad if dtype.is_floating_point else None)

    def output(self, dtype, rows, width, ld, name=None, pad_zero=False):
        """An output the kernel's contract says it writes completely: left at 0xFF.  pad_zero: the header says the kernel also
        writes the in-row padding, with zeros."""
        return self._carve(name, "out", dtype, rows, width, ld, pad_zero)

    def accumulator(self, host, dtype, rows, width, ld, name=None):
        """An output that is added into (or updated in place): holds `host`, padding stays 0xFF."""
        return self._fill(self._carve(name, "acc", dtype, rows, width, ld), host, None)

    def scratch(self, nbytes, name=None):
        """A workspace: its contents are the kernel's business, only the bytes around it are checked."""
        return self._carve(name, "ws", torch.uint8, 1, nbytes, nbytes)

    def vector(self, host, dtype, name=None, kind="in"):
        host = torch.as_tensor(host).reshape(-1)
        n = host.numel()
        return self.operand(host, dtype, 1, n, n, name=name) if kind == "in" else self.accumulator(host, dtype, 1, n, n, name=name)

    def freeze(self, *slots):
        """The results of one launch become read-only inputs of the next launch on the same arena (o and lse of the attention
        forward pass for its backward pass): from the next arm() on, check() requires them bitwise unchanged."""
        for s in slots:
            assert s.arena is self and s.kind in ("out", "acc", "in")
            s.kind = "in"

    # ------------------------------------------------------------------ checking
    def arm(self):
        """Snapshot right before a launch (check() compares with it); calling it again re-arms for the next launch on the same arena."""
        if self.device != "cpu":
            torch.cuda.synchronize()
        self.snap = self.buf.cpu().numpy().copy()
        return self

    def _where(self, s, byte):
        """Position of an arena byte relative to window s, in elements of s."""
        if byte < s.start:
            return "%d element(s) before (row 0, column 0)" % (-(-(s.start - byte) // s.esize))
        idx = (byte - s.start) // s.esize
        return "(row %d, column %d)" % (idx // s.ld, idx % s.ld)

    def check(self):
        if self.device != "cpu":
            torch.cuda.synchronize()
        assert getattr(self, "snap", None) is not None, "arena.arm() must run before the launch"
        now = self.buf.cpu().numpy()
        # 1. guards: everything outside the windows is still 0xFF
        edges = [(None, 0, 0)] + [(s, s.start, s.start + s.nbytes) for s in self.slots] + [(None, now.size, now.size)]
        for (prev, _, lo), (nxt, hi, _) in zip(edges[:-1], edges[1:]):
            gap = now[lo:hi]
            bad = np.flatnonzero(gap != 0xFF)
            if bad.size:
                b = lo + int(bad[0])
                msg = "guard band overwritten at arena byte %d (value 0x%02x):" % (b, int(now[b]))
                if prev is not None:
                    msg += " %d bytes AFTER the window of '%s', its element %s;" % (b - lo, prev.name, self._where(prev, b))
                if nxt is not None:
                    msg += " %d bytes BEFORE the window of '%s': %s" % (hi - b, nxt.name, self._where(nxt, b))
                raise AssertionError(msg)
        for s in self.slots:
            w_now = now[s.start:s.start + s.nbytes].reshape(s.rows, s.ld * s.esize)
            w_old = self.snap[s.start:s.start + s.nbytes].reshape(s.rows, s.ld * s.esize)
            if s.kind == "ws":
                continue
            if s.kind == "in":
                # 2a. inputs are read-only
                bad = np.argwhere(w_now != w_old)
                if bad.size:
                    r, c = bad[0]
                    raise AssertionError("input '%s' was written at (row %d, column %d)%s" % (
                        s.name, r, c // s.esize, " -- in-row padding" if c // s.esize >= s.width else ""))
                continue
            # 2b. in-row padding of outputs: bitwise what it was, or zero where the header says the kernel writes it
            if s.ld > s.width:
                p_now, p_old = w_now[:, s.width * s.esize:], w_old[:, s.width * s.esize:]
                bad = np.argwhere(p_now != 0) if s.pad_zero else np.argwhere(p_now != p_old)
                if bad.size:
                    r, c = bad[0]
                    raise AssertionError("output '%s': in-row padding %s at (row %d, column %d), inside the window, after the logical row"
                                         % (s.name, "is not zero" if s.pad_zero else "was overwritten", r, s.width + c // s.esize))
            # 3. logical window: nothing left at the fill pattern, nothing non-finite
            lg = w_now[:, :s.width * s.esize]
            if s.kind == "out":
                left = (lg.reshape(s.rows, s.width, s.esize) == 0xFF).all(-1)
                if left.any():
                    r, c = np.argwhere(left)[0]
                    raise AssertionError("output '%s': element (row %d, column %d) was never written (still the 0xFF pattern)" % (s.name, r, c))
            if s.dtype.is_floating_point:
                v = torch.from_numpy(now[s.start:s.start + s.nbytes].copy()).view(s.dtype).view(s.rows, s.ld)[:, :s.width]
                nf = ~torch.isfinite(v.float())
                if nf.any():
                    r, c = nf.nonzero()[0].tolist()
                    raise AssertionError("output '%s': element (row %d, column %d) is %s: padding or a neighbour's bytes reached a stored value"
                                         % (s.name, r, c, v[r, c].item()))
        self.snap = None


# ---------------------------------------------------------------------------------------- the per-element bound
def seq_fp32_matmul(a, b):
    """a [M, K] . b [K, N], accumulated over k in float32 STRICTLY in order (one rank-1 update per k); returns float64."""
    a32, b32 = a.to(torch.float32), b.to(torch.float32)
    acc = torch.zeros(a32.shape[0], b32.shape[1], dtype=torch.float32)
    for k in range(a32.shape[1]):
        acc += a32[:, k:k + 1] * b32[k:k + 1, :]
    return acc.double()


def q_seq_of(a, b):
    """max_ij |seq - ref| / S for a [M, K], b [K, N] given in float64 (values as rounded to the compute dtype); also ref and S."""
    ref = a @ b
    S = a.abs() @ b.abs()
    q = ((seq_fp32_matmul(a, b) - ref).abs() / S.clamp_min(1e-300)).max().item()
    return q, ref, S


def acc_factor(q_seq, K):
    return min(SEQ_MARGIN * q_seq, (K + 8) * EPS24)


def gemm_bound(a, b, extra=None):
    """(ref, S, factor): float64 product, S = |a|.|b| + extra, and the accumulation factor; the accumulation term is factor * S."""
    q, ref, S = q_seq_of(a, b)
    if extra is not None:
        S = S + extra
    return ref, S, acc_factor(q, a.shape[1])


def colsum_bound(x, start=None):
    """Column sums of x [rows, cols] (float64 values as stored) added onto `start` [cols]: (ref, S, factor) with the summands
    start, x[0], x[1], ... in that order (the start value is the first summand: K = rows + 1)."""
    if start is not None:
        x = torch.cat([start.reshape(1, -1).double(), x], 0)
    ones = torch.ones(1, x.shape[0], dtype=torch.float64)
    return tuple(t.reshape(-1) if torch.is_tensor(t) else t for t in gemm_bound(ones, x))


def assert_within(out, ref, acc, bf16_out, what="", extra=0.0):
    """|out - ref|_ij <= acc_ij (+ extra) for an fp32 output, 2^-8 |ref_ij| + acc_ij (+ extra) for a bf16 output."""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    lim = acc + extra + (BF16_OUT * ref.abs() if bf16_out else 0.0)
    err = (out - ref).abs()
    bad = ~(err <= lim)               # (a NaN fails)
    if bad.any():
        idx = tuple(bad.nonzero()[0].tolist())
        worst = (err / lim.clamp_min(1e-300)).max().item()
        raise AssertionError("%s: element %s is %.9g, reference %.9g: error %.3g > limit %.3g (worst error/limit of the case %.3g, %d of %d elements)"
                             % (what, idx, out[idx].item(), ref[idx].item(), err[idx].item(), lim[idx].item(), worst, int(bad.sum()), bad.numel()))
    return (err / lim.clamp_min(1e-300)).max().item()


def f32_eval_allowance(fn, x64):
    """4 x the deviation of `fn` evaluated in float32 (numpy) from its float64 value on the same arguments, max over the case."""
    x = np.asarray(x64, dtype=np.float64)
    return 4.0 * float(np.abs(fn(x.astype(np.float32)).astype(np.float64) - fn(x)).max())


def rowwise_rel_err(out, ref):
    """Per row: max |out - ref| over that row's own largest |ref|; returns the worst row's value."""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    return ((out - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-30)).max().item()


# ---------------------------------------------------------------------------------------- Adam: reference, bound, inputs
U24 = 2.0 ** -24              # unit roundoff of fp32: one correctly rounded primitive is off by at most U24 |result|
TINY = 2.0 ** -126            # the smallest normal fp32: what a flushed subnormal result can lose
ADAM_EDGE_SEGMENTS = (("b", 260), ("c", 260), ("d", 516), ("e", 260), ("f", 132), ("g", 260))


def _np64(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def _w32(x):
    """An fp32 ABI argument as the kernel holds it, widened to float64."""
    return float(np.float32(x))


def adam_alpha(lr, beta1, beta2, step):
    """float32(lr * sqrt(1 - beta2^t) / (1 - beta1^t)) evaluated in float64 on the fp32 arguments and rounded once, as the host
    wrappers of cmp_k_adam / cmp_k_adam_dev do (beta^t underflows to 0 for a large t: alpha = lr)."""
    lr, b1, b2, t = _w32(lr), _w32(beta1), _w32(beta2), float(int(step))
    with np.errstate(all="ignore"):
        return float(np.float32(lr * np.sqrt(1.0 - np.power(b2, t)) / (1.0 - np.power(b1, t))))


def adam_reference(p0, g, m0, v0, lr, beta1, beta2, eps, step, factor):
    """Keras-formulation Adam (eps OUTSIDE the bias correction) in float64 -> (p1, m1, v1), numpy float64.

        gg = g * factor;  m1 = beta1 m0 + (1 - beta1) gg;  v1 = beta2 v0 + (1 - beta2) gg^2;  p1 = p0 - alpha m1 / (sqrt(v1) + eps)

    The hyper-parameters and `factor` are the fp32 values the ABI receives, widened; 1 - beta is formed in float64 from the widened
    beta (the kernel's fp32 difference 1.0f - beta is exact for beta in [0.5, 1], Sterbenz); alpha is `adam_alpha`."""
    p0, g, m0, v0 = _np64(p0), _np64(g), _np64(m0), _np64(v0)
    b1, b2, e, f = _w32(beta1), _w32(beta2), _w32(eps), _w32(factor)
    alpha = adam_alpha(lr, beta1, beta2, step)
    gg = g * f
    m1 = b1 * m0 + (1.0 - b1) * gg
    v1 = b2 * v0 + (1.0 - b2) * gg * gg
    return p0 - alpha * m1 / (np.sqrt(v1) + e), m1, v1


def adam_bounds(p0, g, m0, v0, lr, beta1, beta2, eps, step, factor):
    """Per-element limits (lim_p, lim_m, lim_v) for an fp32 evaluation of `adam_reference`, by first-order propagation with every
    fp32 primitive (multiply, add, divide, square root; an fma only removes a rounding) within one ulp, u = 2^-24 of its result --
    hipcc divides and takes square roots correctly rounded unless fast-math is on, and the build passes only -O3:

        gg   = g factor
        dm   = 3u (|beta1 m0| + |(1 - beta1) gg|) + tiny                  gg, the two products, the sum
        dv   = 4u (beta2 v0 + (1 - beta2) gg^2) + tiny
        dsq  = min(dv / (2 sqrt(v1)), sqrt(dv)) + u sqrt(v1)              the second form where v1 is (next to) zero
        den  = sqrt(v1) + eps,   dden = dsq + u den
        U    = alpha m1 / den
        dU   = alpha (dm / den + |m1| dden / den^2) + 3u |U| + tiny       the product, the quotient, alpha's own rounding
        dp   = dU + u |p0 - U|

    and the limits are 2 dm, 2 dv, 2 dp: a margin of 2 over the derivation.  tiny = 2^-126 covers a flushed subnormal.
    Measured on the CPU (tests/test_kernel_checks_host.py, the unfused numpy-fp32 statement of the kernel on `adam_inputs`, factors
    1, 0.5, 1/3, t = 1, 2, 7, 1000, 10^6, 2^31 + 5): worst error / limit 0.50 for p, 0.31 for m, 0.38 for v (factor 1/3; 0.24 for v at
    factor 0.5, where g factor is exact)."""
    p0, g, m0, v0 = _np64(p0), _np64(g), _np64(m0), _np64(v0)
    b1, b2, e, f = _w32(beta1), _w32(beta2), _w32(eps), _w32(factor)
    alpha = adam_alpha(lr, beta1, beta2, step)
    _, m1, v1 = adam_reference(p0, g, m0, v0, lr, beta1, beta2, eps, step, factor)
    gg = g * f
    dm = 3 * U24 * (np.abs(b1 * m0) + np.abs((1.0 - b1) * gg)) + TINY
    dv = 4 * U24 * (b2 * v0 + (1.0 - b2) * gg * gg) + TINY
    sq = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        dsq = np.minimum(np.where(sq > 0, dv / (2 * sq), np.inf), np.sqrt(dv)) + U24 * sq
    den = sq + e
    dden = dsq + U24 * den
    U = alpha * m1 / den
    dU = alpha * (dm / den + np.abs(m1) * dden / (den * den)) + 3 * U24 * np.abs(U) + TINY
    dp = dU + U24 * np.abs(p0 - U)
    return 2 * dp, 2 * dm, 2 * dv


def adam_inputs(factor=1.0, seed=9, n_generic=1028):
    """One vector in segments, every length a multiple of 4, the default total (2716) no multiple of 1024 and more than one block:

        a  the generic draw of the older Adam tests: p0 ~ N(0, 1), g ~ 0.1 N(0, 1), m0 ~ 0.01 N(0, 1), v0 ~ U(0, 0.01)
        b  p0 = 0 exactly, generic state: the update is read off p1 at full fp32 resolution, not through the rounding of p
        c  m0 = v0 = 0, generic g: the first step of a run
        d  m0 = v0 = 0, p0 = 0, |g factor| log-uniform in [1e-9, 1e-4], random sign: on a first step sqrt(v1) = sqrt(1 - beta2) |g factor|,
           0.0003 eps to 30 eps (eps = 1e-7), where the placement of eps decides the value ([1e-9, 1e-6] alone would end at 0.3 eps)
        e  g = 0, non-zero state: pure decay
        f  g = 0 and m0 = v0 = 0: p bitwise unchanged, m = v = 0, nothing non-finite
        g  |g| log-uniform up to 1e4

    -> (dict of float32 CPU tensors p0, g, m0, v0; dict name -> slice).  The edge segments follow the generic one, so with a large
    n_generic they sit where a grid-stride loop takes its later trips."""
    assert n_generic % 4 == 0
    n = n_generic + sum(k for _, k in ADAM_EDGE_SEGMENTS)
    gen = torch.Generator().manual_seed(seed)
    p0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1
    m0, v0 = torch.randn(n, generator=gen) * 0.01, torch.rand(n, generator=gen) * 0.01
    seg, lo = {"a": slice(0, n_generic)}, n_generic
    for name, k in ADAM_EDGE_SEGMENTS:
        seg[name] = slice(lo, lo + k)
        lo += k

    def signed_log_uniform(k, lo10, hi10):
        mag = 10.0 ** (lo10 + (hi10 - lo10) * torch.rand(k, generator=gen, dtype=torch.float64))
        return mag * (torch.randint(0, 2, (k,), generator=gen).double() * 2 - 1)
    p0[seg["b"]] = 0
    m0[seg["c"]] = 0; v0[seg["c"]] = 0
    m0[seg["d"]] = 0; v0[seg["d"]] = 0; p0[seg["d"]] = 0
    g[seg["d"]] = (signed_log_uniform(seg["d"].stop - seg["d"].start, -9, -4) / _w32(factor)).float()
    g[seg["e"]] = 0
    g[seg["f"]] = 0; m0[seg["f"]] = 0; v0[seg["f"]] = 0
    g[seg["g"]] = signed_log_uniform(seg["g"].stop - seg["g"].start, 0, 4).float()
    assert n % 4 == 0 and all((s.stop - s.start) % 4 == 0 for s in seg.values())
    return {"p0": p0, "g": g, "m0": m0, "v0": v0}, seg


def bf16_truncated(t):
    """fp32 -> bf16 by dropping the low 16 bits: what a shadow store must NOT do."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def adam_check(inp, seg, p, m, v, shadow, lr, beta1, beta2, eps, step, factor, what="adam", ref_lim=None):
    """Everything the kernel-level Adam cases assert about one launch on `adam_inputs`, given the arrays read back (CPU tensors):
    p, m, v per element inside `adam_bounds` of `adam_reference`; segment f untouched bit for bit with m = v = 0; with lr = 0 every
    p bitwise unchanged while m and v moved; the bf16 shadow the round-to-nearest-even image of the p that was stored, on values
    where truncation would differ.  ref_lim: (adam_reference, adam_bounds) of exactly these arguments, where a large case shares
    them.  -> {"p", "m", "v"}: the worst error / limit of each array."""
    args = (inp["p0"], inp["g"], inp["m0"], inp["v0"], lr, beta1, beta2, eps, step, factor)
    ref, lim = ref_lim if ref_lim is not None else (adam_reference(*args), adam_bounds(*args))
    worst = {}
    for name, out, r, l in (("m", m, ref[1], lim[1]), ("v", v, ref[2], lim[2]), ("p", p, ref[0], lim[0])):
        worst[name] = assert_within(out, torch.from_numpy(r), torch.from_numpy(l), False, "%s: %s at step %d" % (what, name, step))
    f = seg["f"]
    assert same_bits(p[f], inp["p0"][f]), "%s: a parameter with g = m = v = 0 was touched" % what
    assert bool((m[f] == 0).all()) and bool((v[f] == 0).all()), "%s: g = m0 = v0 = 0 must leave m = v = 0" % what
    if float(np.float32(lr)) == 0.0:
        assert same_bits(p, inp["p0"]), "%s: lr = 0 must leave every parameter bitwise unchanged" % what
        assert not torch.equal(m, inp["m0"]) and not torch.equal(v, inp["v0"]), "%s: lr = 0 must still move m and v" % what
    if shadow is not None:
        rne = p.to(torch.bfloat16)
        assert bool((rne != bf16_truncated(p)).any()), "%s: no stored value tells round-to-nearest from truncation" % what
        assert torch.equal(shadow, rne), "%s: the bf16 shadow is not the round-to-nearest-even image of the stored parameters" % what
    return worst
