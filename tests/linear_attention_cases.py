"""Seeded cases, layouts, padding masks and fp64 references of the linear-attention edge tests: shared by
tests/test_linear_attention_cases_cpu.py (which judges them on the host alone) and tests/test_gpu_linear_attention_edges.py.  Nothing
here touches a device; operands and references are built once per case and frozen (lru_cache: the tests clone before they modify).

The reference, ref_attention, is a float64 restatement of LinearAttention.forward (attentions.py:20-47) on operands that are ALREADY
rounded to the kernel's input dtype and ALREADY mapped through elu + 1 (the projection GEMM's epilogue does both in the product), so
it accounts for the input rounding and for nothing else.  The bars are the project's existing ones (tests/test_gpu_kernels.py): BAR_OUT
of max|ref| by OUTPUT dtype, BAR_STATE of max|ref| for the fp32 KV / Ksum state.

A case names the route it is meant for; route() restates the dispatch of ops.linear_attention / csrc/linear_attention.hip so that the
CPU test can hold every case to its claim (and list the template instances the cases reach)."""
import collections
import functools

import torch
import torch.nn.functional as F

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTS = ("fp32", "bf16", "fp16")
BAR_OUT = {"bf16": 1e-2, "fp16": 1e-2 / 8, "fp32": 1e-5}    # _ht(dt, 1e-2, 1e-5) of tests/test_gpu_kernels.py
BAR_STATE = 1e-5
EPS = 1e-6
SENTINEL = 7.0                                               # foreign columns of a wider buffer: never read, never written
CH_PLAIN, CH_MFMA, APPLY_ROWS = 128, 256, 64                 # S rows per partial (la_kv_kernel / the MFMA kernels), L rows per apply workgroup
PAIRS = (("fp32", "fp32"), ("bf16", "bf16"), ("bf16", "fp32"), ("fp32", "bf16"), ("fp16", "fp16"), ("fp16", "fp32"), ("fp32", "fp16"))

# the two S > 4096 state cases: fp32 accumulation over 33 chunks.  LONG_S_FP32_DEV is the deviation of a plain fp32 torch evaluation
# of the state from ref_state, of max|ref|: measured on the host at 3.8e-7 (S = 8193) and 4.5e-7 (S = 4097), recorded here rounded up
# to 1e-6 because the order of a host einsum's additions depends on the build and its threads (tests/test_linear_attention_cases_cpu.py
# holds the measurement to it); the GPU bar is max(BAR_STATE, 4 x that): 4 for a different summation tree.
LONG_S = {"mfma": (1, 8193, 8, 32), "plain": (1, 4097, 4, 32)}      # (nb, S, H, D): 33 chunks of 256 / of 128
LONG_S_FP32_DEV = {"mfma": 1.0e-6, "plain": 1.0e-6}


def long_s_bar(kind):
    return max(BAR_STATE, 4 * LONG_S_FP32_DEV[kind])


Case = collections.namedtuple("Case", "id route nb L S H D dt odt mask garbage layout seed")


def route(nb, L, S, H, D, dt, layout="plain"):
    """-> (route, kv kernel, apply kernel) as ops.linear_attention and the two entry points dispatch"""
    if H == 8 and D in (16, 32) and L <= 64 and S <= 64:
        return "short", None, "la_short_kernel"
    aligned = layout != "misaligned"         # strided views keep 16-byte bases and pitches (multiples of C >= 16 elements)
    kv = ("la_kv_mfma2_kernel" if dt == "fp32" else "la_kv_h16_kernel") if (H == 8 and D == 32 and aligned) else "la_kv_kernel"
    if H == 8 and D == 32:
        return ("mfma" if aligned else "plain"), kv, "la_apply_mfma_kernel"
    return "plain", kv, "la_apply_kernel"


def nchunk(S, kv_kernel):
    ch = CH_PLAIN if kv_kernel == "la_kv_kernel" else CH_MFMA
    return (S + ch - 1) // ch


def instances(c):
    """the template instances of csrc/linear_attention.hip a case launches (16-bit = one flavour per 16-bit kind)"""
    _, kv, ap = route(c.nb, c.L, c.S, c.H, c.D, c.dt, c.layout)
    i16, o16 = c.dt != "fp32", c.odt != "fp32"
    out = [(ap, c.D, i16, o16)]
    if kv == "la_kv_kernel":
        out.append((kv, c.D, i16))
    return out


# ------------------------------------------------------------------------------------------------------------ masks
def mask_random(nb, n, seed, p=0.7):
    """valid with probability p, independently per row"""
    return torch.rand(nb, n, generator=torch.Generator().manual_seed(seed)) < p


def mask_prefix(nb, n, length):
    """a padding mask: rows [0, length) valid; `length` an int or one per sequence"""
    ln = torch.as_tensor([length] * nb if isinstance(length, int) else list(length))
    return torch.arange(n)[None, :] < ln[:, None]


def mask_prefix_chunks(nb, n, chunks=1):
    """a prefix that ends exactly on a multiple of 256 rows (a chunk boundary of every KV kernel)"""
    assert 256 * chunks < n
    return mask_prefix(nb, n, 256 * chunks)


def mask_chunk_cleared(nb, n, lo=256, hi=512):
    """all valid but rows [lo, hi): one whole 256-row chunk (two 128-row ones) contributes nothing"""
    assert hi <= n
    m = torch.ones(nb, n, dtype=torch.bool)
    m[:, lo:hi] = False
    return m


def mask_sequence_cleared(nb, n, which):
    """all-zero for sequence `which`, all-ones for the others"""
    m = torch.ones(nb, n, dtype=torch.bool)
    m[which] = False
    return m


def build_masks(kind, nb, L, S, seed):
    """(q_mask [nb, L], kv_mask [nb, S]) bool.  The q side mirrors the kv side at the apply kernels' 64-row workgroup."""
    if kind == "random":
        return mask_random(nb, L, seed + 1), mask_random(nb, S, seed + 2)
    if kind == "prefix":          # a different ragged length per sequence, as a padded batch has
        return mask_prefix(nb, L, [L - 1 - (17 * b) % (L - 1) for b in range(nb)]), mask_prefix(nb, S, [S - 1 - (29 * b + 2) % (S - 1) for b in range(nb)])
    if kind in ("prefix256", "prefix512"):
        return mask_prefix(nb, L, APPLY_ROWS * (1 if kind == "prefix256" else 2)), mask_prefix_chunks(nb, S, 1 if kind == "prefix256" else 2)
    if kind == "chunk":
        return mask_chunk_cleared(nb, L, APPLY_ROWS, 2 * APPLY_ROWS), mask_chunk_cleared(nb, S)
    if kind == "seqzero":         # sequence 0: every q row masked; sequence 1: every kv row masked; the last one: all valid
        assert nb >= 3
        qm = mask_random(nb, L, seed + 1)
        qm[0], qm[nb - 1] = False, True
        return qm, mask_sequence_cleared(nb, S, 1)
    raise KeyError(kind)


def garbage_value(dt):
    """what masked rows hold on the device: large and finite (0.5 x the 16-bit dtype's max, 1e30 for fp32).  Not NaN / Inf: the
    reference multiplies by the mask, and 0 * NaN is NaN there by definition."""
    return 1e30 if dt == "fp32" else 0.5 * torch.finfo(TDT[dt]).max


def with_garbage(x, mask, dt):
    """copy of x [nb, n, H, D] with the masked rows overwritten by +-garbage_value (alternating over the channels)"""
    big = torch.full(x.shape[2:], garbage_value(dt))
    big.view(-1)[1::2] *= -1
    y = x.clone()
    y[~mask] = big
    return y


# ------------------------------------------------------------------------------------------------------------ references
def _attention(q, k, v, q_mask, kv_mask, dtype):
    Q, K, V = q.to(dtype), k.to(dtype), v.to(dtype)
    if q_mask is not None:
        Q = Q * q_mask[:, :, None, None]                                  # attentions.py:36
    if kv_mask is not None:
        K = K * kv_mask[:, :, None, None]                                 # :38
        V = V * kv_mask[:, :, None, None]                                 # :39
    S = V.size(1)
    V = V / S                                                             # :42
    KV = torch.einsum("nshd,nshv->nhdv", K, V)                            # :43
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", Q, K.sum(dim=1)) + EPS)        # :44
    return torch.einsum("nlhd,nhdv,nlh->nlhv", Q, KV, Z) * S              # :45


def ref_attention(q, k, v, q_mask=None, kv_mask=None):
    """THE reference: attentions.py:20-47 in float64 on mapped, rounded operands q [nb,L,H,D], k / v [nb,S,H,D] -> [nb,L,H,D]"""
    return _attention(q, k, v, q_mask, kv_mask, torch.float64)


def fp32_attention(q, k, v, q_mask=None, kv_mask=None):
    """the same formula as torch evaluates it in fp32: the reference-side margin the CPU test measures"""
    return _attention(q, k, v, q_mask, kv_mask, torch.float32)


def _state(k, v, kv_mask, dtype):
    K, V = k.to(dtype), v.to(dtype)
    if kv_mask is not None:
        K, V = K * kv_mask[:, :, None, None], V * kv_mask[:, :, None, None]
    nb, S, H, D = K.shape
    KV = torch.einsum("nshd,nshv->nhdv", K, V / S)
    return KV.reshape(nb, H, D * D), K.sum(dim=1)


def ref_state(k, v, kv_mask=None):
    """(KV [nb,H,D*D], Ksum [nb,H,D]) in float64: the layout of the workspace's leading nb*H*(D*D+D) floats"""
    return _state(k, v, kv_mask, torch.float64)


def fp32_state(k, v, kv_mask=None):
    return _state(k, v, kv_mask, torch.float32)


def rel_err(got, ref):
    """max|got - ref| / max|ref|"""
    return (got.double() - ref.double()).abs().max().item() / max(1e-6, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def raw_operands(nb, L, S, H, D, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(nb, n, H, D, generator=g) for n in (L, S, S))


@functools.lru_cache(maxsize=None)
def mapped_operands(nb, L, S, H, D, dt, seed):
    """(Q, K, V) fp32 containers of dt-rounded values, q / k through elu + 1 first (what the kernels are handed)"""
    q, k, v = raw_operands(nb, L, S, H, D, seed)
    r = lambda t: t.to(TDT[dt]).float()   # noqa: E731
    return r(F.elu(q) + 1), r(F.elu(k) + 1), r(v)


@functools.lru_cache(maxsize=None)
def case_inputs(c):
    """(Q, K, V, q_mask, kv_mask) of a case: masks None when the case has none"""
    Q, K, V = mapped_operands(c.nb, c.L, c.S, c.H, c.D, c.dt, c.seed)
    qm, km = build_masks(c.mask, c.nb, c.L, c.S, c.seed) if c.mask else (None, None)
    return Q, K, V, qm, km


@functools.lru_cache(maxsize=None)
def case_ref(c):
    return ref_attention(*case_inputs(c))


@functools.lru_cache(maxsize=None)
def state_operands(nb, S, H, D, dt, seed):
    g = torch.Generator().manual_seed(seed)
    k = (F.elu(torch.randn(nb, S, H, D, generator=g)) + 1).to(TDT[dt]).float()
    v = torch.randn(nb, S, H, D, generator=g).to(TDT[dt]).float()
    return k, v


# ------------------------------------------------------------------------------------------------------------ layouts
LAYOUTS = {   # per operand (pitch in units of C, first column in units of C) -- None: pitch C, column 0
    "plain": {"q": None, "k": None, "v": None, "out": None},
    "strided": {"q": (2, 1), "k": (3, 1), "v": (3, 2), "out": (3, 1)},
}
MISALIGNED_PITCH, MISALIGNED_COL = 260, 4   # 16-bit K / V of C = 256: base 8 bytes past a 16-byte boundary, rows 520 bytes apart


def column_view(x2d, tdt, pitch, col0):
    """host buffer [rows, pitch] of dtype tdt, SENTINEL everywhere but columns [col0, col0 + C), which hold x2d -> (buf, slice)"""
    rows, C = x2d.shape
    assert col0 + C <= pitch
    buf = torch.full((rows, pitch), SENTINEL, dtype=tdt)
    buf[:, col0:col0 + C] = x2d.to(tdt)
    return buf, slice(col0, col0 + C)


def lay_out(name, x2d, tdt, layout):
    """operand `name` (q / k / v / out) of a layout -> (buf, slice)"""
    C = x2d.shape[1]
    if layout == "misaligned" and name in ("k", "v"):
        assert tdt != torch.float32 and C == 256
        return column_view(x2d, tdt, MISALIGNED_PITCH, MISALIGNED_COL)
    spec = LAYOUTS["plain" if layout == "misaligned" else layout][name]
    return column_view(x2d, tdt, C * spec[0], C * spec[1]) if spec else column_view(x2d, tdt, C, 0)


def foreign_columns_untouched(buf_after, sl):
    """bit for bit: every column of `buf_after` outside `sl` still holds SENTINEL"""
    it = {2: torch.int16, 4: torch.int32}[buf_after.element_size()]
    want = torch.full((1,), SENTINEL, dtype=buf_after.dtype).view(it)
    keep = torch.ones(buf_after.shape[1], dtype=torch.bool)
    keep[sl] = False
    return bool((buf_after.cpu().view(it)[:, keep] == want).all())


# ------------------------------------------------------------------------------------------------------------ the cases
def _case(tag, nb, L, S, H, D, dt, odt=None, mask=None, layout="plain", seed=0):
    odt = odt or dt
    r = route(nb, L, S, H, D, dt, layout)[0]
    name = f"{tag}-{nb}x{L}x{S}x{H}x{D}-{dt}" + (f"-to-{odt}" if odt != dt else "") + (f"-{mask}" if mask else "") + ("" if layout == "plain" else f"-{layout}")
    return Case(name, r, nb, L, S, H, D, dt, odt, mask, bool(mask), layout, 4100 + seed)


# routing boundary of ops.linear_attention (L <= 64 and S <= 64): H = 8; nb of 3, 5, 6: the short kernel's four-sequences-per-workgroup tail
ROUTING_SHAPES = ((1, 1, 1), (3, 64, 64), (5, 65, 64), (5, 64, 65), (2, 1, 64), (6, 25, 64))
ROUTING = tuple(_case("route", nb, L, S, 8, D, dt, seed=1) for D in (16, 32) for dt in DTS for (nb, L, S) in ROUTING_SHAPES)

# the plain kernels: every (H, D), S of 1, 1, 2 and 3 chunks of 128, each L with each D; H = 15, D = 32: 63 360 B of LDS, the most that fits
PLAIN_SHAPES = ((2, 65, 65, 4, 32), (2, 130, 257, 4, 32), (3, 130, 128, 1, 32), (2, 65, 129, 1, 32), (2, 65, 257, 2, 16), (3, 130, 129, 2, 16),
                (2, 130, 65, 12, 16), (2, 65, 128, 12, 16), (2, 130, 257, 8, 16), (2, 65, 65, 8, 16), (2, 65, 129, 15, 32))
PLAIN = tuple(_case("plain", *s, dt, seed=2) for s in PLAIN_SHAPES for dt in DTS)
MISALIGNED = tuple(_case("plain", 2, 130, 257, 8, 32, dt, mask=m, layout="misaligned", seed=3) for dt in ("bf16", "fp16") for m in (None, "random"))

# every (input, output) dtype pair of la_short (D = 16, 32), la_apply_mfma and la_apply_kernel (D = 32, 16)
PAIR_SHAPES = ((5, 25, 33, 8, 16), (5, 33, 25, 8, 32), (2, 130, 257, 8, 32), (2, 65, 129, 4, 32), (2, 65, 129, 2, 16))
DTYPE_PAIRS = tuple(_case("pair", *s, a, b, seed=4) for s in PAIR_SHAPES for (a, b) in PAIRS)

STRIDED = tuple(_case("strided", *s, dt, layout="strided", seed=5) for s in PAIR_SHAPES for dt in DTS)

# masks with garbage in the masked rows.  The 256-row builders need S >= 512: they do not exist on the short route (S <= 64).
MASK_SHAPES = (
    ((6, 25, 33, 8, 16), ("random", "prefix", "seqzero")), ((5, 33, 25, 8, 32), ("random", "prefix", "seqzero")),          # short
    ((2, 200, 140, 8, 32), ("random", "prefix")), ((2, 300, 513, 8, 32), ("chunk", "prefix256", "prefix512")),             # MFMA
    ((3, 70, 257, 8, 32), ("seqzero", "random")),
    ((2, 130, 257, 4, 32), ("random", "prefix", "prefix256")), ((2, 130, 513, 2, 16), ("chunk", "prefix512")),             # plain
    ((3, 65, 129, 12, 16), ("seqzero",)),
)
MASKED = tuple(_case("mask", *s, dt, mask=m, seed=6) for (s, kinds) in MASK_SHAPES for m in kinds for dt in DTS)

ALL = ROUTING + PLAIN + MISALIGNED + DTYPE_PAIRS + STRIDED + MASKED
assert len({c.id for c in ALL}) == len(ALL)

# masked batch invariance of the state in the 512-row workgroup shape (16-bit) and of la_kv_mfma2_kernel (fp32)
INVARIANCE = (130, 257)
