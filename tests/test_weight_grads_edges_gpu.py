"""GPU: the weight-gradient kernels at the edges of their K-ranges, against fp64 and with exact point counts.

sn_weight_grads reaches five kernel families (csrc/sn_dw_f32.hip, sn_dw_bf16.hip, sn_dw_narrow_bf16.hip with and without
SN_DTYPE_EMB_BF16, the two-workgroup narrow fp32 kernel and the generic dw_kernel of sn_dw.hip); all of them stream 16-point chunks through
an LDS ring with a prologue of several chunks, counted waits, clamped over-run copies and -- two of them -- pair / quad bodies with a tail
statement.  The row counts of tests.helpers.DW_EDGE_ROWS put K-ranges of 1..8 chunks (shorter than, as long as and longer than every
prologue; odd and 1..3 chunk tails) into the first and the last range of a problem of every launch group, and one size wraps the 16-deep
rings; test_sweep_reaches_the_edges proves that from the plan the library really runs (sn_weight_grads_plan), so a retuned cost table
cannot quietly move the sweep off the edges.  In every call the workspace is filled with NaN bytes, the outputs of accumulate=0 calls
with NaN, and the columns of emb the header calls never-read hold NaN: an unwritten partial or a stray read shows as a non-finite gradient.

  (a) random operands against fp64 matmuls of the values the kernel consumes, at the bars of test_weight_grads_entry_vs_fp64_contractions;
  (b) every point exactly once: all-ones operands must give float(rows) in every element, and single-row operands of small integers the
      fp64 outer product, both bit for bit in every arithmetic (integers below 2^24, zero lo parts);
  (c) the raw sn_dw_gemm entry (dw_kernel alone) with explicit ranges [k0, k1), k0 != 0, NaN rows around them."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from sinnerf_amd import _lib                                                                    # noqa: E402
from tests import helpers as H                                                                  # noqa: E402
from tests.test_parity_gpu import dev                                                           # noqa: E402
from tests.test_training_kernels_system_gpu import _emb_dir_pos, _emb_xyz_pos                   # noqa: E402

MODES = {"fp32": _lib.SN_DTYPE_F32, "bf16": _lib.SN_DTYPE_BF16, "bf16_state": _lib.SN_DTYPE_BF16_STATE,
         "bf16_state_emb16": _lib.SN_DTYPE_BF16_STATE | _lib.SN_DTYPE_EMB_BF16, "bf16x3": _lib.SN_DTYPE_BF16X3}
NAN = float("nan")


def _nan_bytes(shape, dtype):
    """a tensor whose every byte is 0xFF: NaN in fp32 and in bf16, also in both halves of a bf16x3 (hi, lo) pair"""
    t = torch.empty(shape, dtype=dtype, device=dev())
    t.view(torch.uint8).fill_(0xFF)
    return t


def _x3_split(x):
    hi = x.bfloat16()
    return hi, (x - hi.float()).bfloat16()


def _x3_encode(x):
    """tests.helpers.x3_state_encode on the device: fp32 values (..., 256) -> split rows, as float32 bit patterns"""
    hi, lo = _x3_split(x)
    sh = tuple(x.shape[:-1])
    out = torch.stack([hi.reshape(sh + (32, 8)), lo.reshape(sh + (32, 8))], dim=-2)
    return out.reshape(sh + (512,)).contiguous().view(torch.float32)


def _x3_value(x):
    """the fp64 value hi + lo an x3 slot holds for the fp32 value x"""
    hi, lo = _x3_split(x)
    return hi.double() + lo.double()


def test_device_x3_encoder_is_the_helpers_one():
    x = torch.randn((3, 40, 256), device=dev()) * torch.logspace(-6, 6, 40, device=dev())[None, :, None]
    x[0, 0, :8] = torch.tensor([0.0, -0.0, 1.0, -7.0, 3.0e38, 1e-30, 255.0, 257.0], device=dev())
    want = H.x3_state_encode(x.cpu().numpy())
    assert np.array_equal(_x3_encode(x).cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(_x3_value(x).cpu().numpy(), H.x3_state_decode(want).astype(np.float64))


def _store(mode, A, E, G):
    """fp32 values A (10, rows, 256), E (rows, 128: columns [0, 63) and [64, 91) live), G (10, rows, 256) -> the state arrays as
    sn_weight_grads(mode) reads them, and what the reference contracts: (acts, emb, G), (values consumed: A, E, G), G values as stored
    (their sums are the bias gradients in every mode)"""
    rows = E.shape[0]
    if mode == "bf16x3":                                          # slots 0..8 as (hi, lo) pairs; slot 9 and emb fp32, split in registers
        acts, Gs = A.clone(), G.clone()
        acts[:9], Gs[:9] = _x3_encode(A[:9]), _x3_encode(G[:9])
        cA, cG = A.double(), G.double()
        cA[:9], cG[:9] = _x3_value(A[:9]), _x3_value(G[:9])
        cE, sG = E, cG
    elif mode in ("bf16_state", "bf16_state_emb16"):
        acts, Gs = A.bfloat16(), G.bfloat16()
        cA, cE, cG = acts, E.bfloat16(), Gs
        sG = cG
    elif mode == "bf16":                                          # fp32 state, operands rounded on their way to the MFMA
        acts, Gs = A, G
        cA, cE, cG, sG = A.bfloat16(), E.bfloat16(), G.bfloat16(), G
    else:
        acts, Gs, cA, cE, cG, sG = A, G, A, E, G, G
    if mode == "bf16_state_emb16":                                # bf16 in K-slot order; the unused positions and [96, 128) are never read
        emb = torch.full((rows, 128), NAN, dtype=torch.bfloat16, device=dev())
        emb[:, [_emb_xyz_pos(c) for c in range(63)]] = E[:, :63].bfloat16()
        emb[:, [64 + _emb_dir_pos(c) for c in range(27)]] = E[:, 64:91].bfloat16()
    else:                                                         # columns 63 and 91..127 are never written by the forward
        emb = E.clone()
        emb[:, 63] = NAN
        emb[:, 91:] = NAN
    return (acts.contiguous(), emb.contiguous(), Gs.contiguous()), (cA, cE, cG), sG


def _reference(consumed, sG):
    """the 24 gradients in fp64: weights from the consumed values, biases from the stored G"""
    cA, cE, cG = consumed
    ref = H.weight_grads_reference(cA, cE, cG)
    if sG is not cG:
        refb = H.weight_grads_reference(cA, cE, sG)
        ref = [rb if i % 2 else r for i, (r, rb) in enumerate(zip(ref, refb))]
    return [r.reshape(s) for r, s in zip(ref, H.RAW_SHAPES)]


def _run(mode, state, rows, accumulate=0, prefill=NAN):
    """one sn_weight_grads call on a NaN-filled workspace -> the 24 outputs (all finite, or the test fails)"""
    code = MODES[mode]
    nbytes = _lib.lib.sn_weight_grads_workspace_bytes(rows, code)
    assert nbytes > 0, (mode, rows, nbytes)
    ws = _nan_bytes((int(nbytes),), torch.uint8)
    outs = [torch.full(s, prefill, device=dev()) for s in H.RAW_SHAPES]
    arr = (ctypes.c_void_p * _lib.N_RAW_TENSORS)(*[o.data_ptr() for o in outs])
    acts, emb, G = state
    _lib.check(_lib.lib.sn_weight_grads(_lib.ptr(acts), _lib.ptr(emb), _lib.ptr(G), rows, code, _lib.ptr(ws), arr, accumulate, None),
               "sn_weight_grads")
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert bool(torch.isfinite(o).all()), (mode, rows, "output", i, "non-finite elements", int((~torch.isfinite(o)).sum()))
    return outs


def _mismatch(got, want):
    """None if bit-equal, else where and by how much the first of the wrong elements is off"""
    if torch.equal(got, want):
        return None
    bad = (got != want).reshape(-1).nonzero().reshape(-1)
    j = int(bad[0])
    return {"wrong": int(bad.numel()), "of": got.numel(), "first": j, "got": float(got.reshape(-1)[j]), "want": float(want.reshape(-1)[j])}


@pytest.mark.parametrize("mode", list(MODES))
def test_sweep_reaches_the_edges(mode):
    """The proof that the sweep reaches the edges and not merely many sizes: over DW_EDGE_ROWS, the plan the library runs has a FIRST and a
    LAST K-range of every chunk count 1..8 among the problems of each launch group and among the 256 x 256 problems, and at
    DW_EDGE_WRAP_ROWS a narrow problem whose ranges are longer than the 16-deep ring."""
    reach, longest_narrow = H.dw_edge_reach(MODES[mode])
    two = mode in ("fp32", "bf16_state", "bf16_state_emb16")
    assert set(reach) == {("group", 0), ("variant0",)} | ({("group", 1)} if two else set())
    for key, (first, last) in reach.items():
        assert first >= set(range(1, 9)), (mode, key, "first ranges", sorted(first))
        assert last >= set(range(1, 9)), (mode, key, "last ranges", sorted(last))
    assert longest_narrow > 16, (mode, longest_narrow)
    for c in (1, 2, 3, 4, 5, 6, 7):                               # one range of c chunks per problem
        assert all(q["ns"] == 1 for q in H.dw_plan(16 * c, MODES[mode])), (mode, c)


def _random_values(rows, seed):
    g = torch.Generator(device=dev())
    g.manual_seed(seed)
    A = torch.randn((10, rows, 256), device=dev(), generator=g)
    # a non-zero mean keeps the one- and three-element bias sums (sigma, rgb) away from cancellation: a norm-wise bar on a single sum of
    # zero-mean terms measures how close to zero that sum happened to fall, not the kernel
    G = torch.randn((10, rows, 256), device=dev(), generator=g) * 0.1 + 0.02
    E = torch.randn((rows, 128), device=dev(), generator=g)
    A[9, :, 128:] = 0
    G[9, :, 132:160] = 0                                          # the head block carries 4 live columns (sn_mlp_bwd.hip)
    return A, E, G


@pytest.mark.parametrize("rows", H.DW_EDGE_ROWS)
@pytest.mark.parametrize("mode", list(MODES))
def test_random_operands_vs_fp64(mode, rows):
    """(a) norm-wise 1e-5 for fp32 and for every bias sum, 2e-5 for the bf16-operand modes and bf16x3 (the bars of
    test_weight_grads_entry_vs_fp64_contractions, which were sized for 4144 points), at every size of the sweep including the 16656-row
    one.  Measured on an MI355X, worst output over all sizes (weights / biases), and at 16656 rows alone:
        fp32              4.2e-07 / 2.1e-07    4.2e-07 / 2.1e-07
        bf16              3.1e-07 / 2.6e-07    3.1e-07 / 8.9e-08
        bf16_state        2.0e-07 / 1.6e-07    2.0e-07 / 1.6e-07
        bf16_state_emb16  2.0e-07 / 1.8e-07    2.0e-07 / 1.8e-07
        bf16x3            5.2e-06 / 2.6e-07    4.5e-06 / 1.6e-07   (the dropped lo x lo term and the register split of slot 9 / emb)
    -- every mode stays under the 4144-point bars at 16656 rows, so no bar was re-measured for that size."""
    state, consumed, sG = _store(mode, *_random_values(rows, 1000 + rows))
    ref = _reference(consumed, sG)
    outs = _run(mode, state, rows)
    errs = [((o.double() - r).norm() / r.norm()).item() for o, r in zip(outs, ref)]
    print("dw-edges random %s rows=%d worst weight %.3e worst bias %.3e" % (mode, rows, max(errs[0::2]), max(errs[1::2])))
    for i, e in enumerate(errs):
        assert e < (1e-5 if mode == "fp32" or i % 2 else 2e-5), (mode, rows, i, e)


def _ones_values(rows):
    A = torch.ones((10, rows, 256), device=dev())
    G = torch.ones((10, rows, 256), device=dev())
    E = torch.ones((rows, 128), device=dev())
    A[9, :, 128:] = 0
    G[9, :, 132:160] = 0
    return A, E, G


@pytest.mark.parametrize("rows", H.DW_EDGE_ROWS)
@pytest.mark.parametrize("mode", list(MODES))
def test_counting_probe(mode, rows):
    """(b) all-ones operands: every weight and every bias gradient is the number of points, exactly -- a chunk consumed twice or not
    at all, a range that is skipped, a stale partial is off by a multiple of 16 (or is NaN).  Then accumulate=1 onto 0.25."""
    state, consumed, sG = _store(mode, *_ones_values(rows))
    ref = [r.float() for r in _reference(consumed, sG)]
    for r in ref:
        assert bool((r == float(rows)).all())
    for i, (o, r) in enumerate(zip(_run(mode, state, rows), ref)):
        assert _mismatch(o, r) is None, (mode, rows, "output", i, _mismatch(o, r))
    for i, (o, r) in enumerate(zip(_run(mode, state, rows, accumulate=1, prefill=0.25), ref)):
        assert _mismatch(o, r + 0.25) is None, (mode, rows, "accumulate, output", i, _mismatch(o, r + 0.25))


def _integer_rows(p):
    """one point row of small signed integers (exact in bf16, zero lo parts), non-zero in every 32-column tile"""
    col = torch.arange(256, device=dev())
    s = torch.arange(10, device=dev())[:, None, None]
    G = (((p + 3 * col[None, None, :] + s) % 15) - 7).float()
    A = (((2 * p + 5 * col[None, None, :] + 3 * s) % 13) - 6).float()
    E = (((p + 7 * col[None, :128]) % 11) - 5).float()
    A[9, :, 128:] = 0
    G[9, :, 132:160] = 0
    return A, E, G


@pytest.mark.parametrize("mode", list(MODES))
def test_position_probes(mode):
    """(b) one live point row p at a time, at the boundaries of the K-ranges the library's plan gives the W1 (256 x 256) and the rgb
    (32 x 128) problem: every gradient must be the outer product of that row, bit for bit -- this names the point that went missing,
    arrived twice or was read from the wrong ring slot."""
    W1, RGB = 1, 13                                               # problems in launch order (csrc/sn_dw.hip build_plan)
    for rows in [16 * c for c in (1, 3, 7, 9, 33)] + [H.DW_EDGE_WRAP_ROWS]:
        plan = H.dw_plan(rows, MODES[mode])
        assert plan[W1]["variant"] & 0xff == 0 and plan[RGB]["variant"] & 0xff == 5
        pers = {plan[W1]["per"], plan[RGB]["per"]}
        points = sorted({p for per in pers for p in (0, 15, 16, per - 1, per, rows - 16, rows - 1) if 0 <= p < rows})
        zeros = (torch.zeros((10, rows, 256), device=dev()), torch.zeros((rows, 128), device=dev()), torch.zeros((10, rows, 256), device=dev()))
        (acts, emb, G), _, _ = _store(mode, *zeros)
        del zeros
        for p in points:
            (ra, re, rg), consumed, sG = _store(mode, *_integer_rows(p))
            ref = [r.float() for r in _reference(consumed, sG)]
            blank = emb[p].clone()
            acts[:, p], emb[p], G[:, p] = ra[:, 0], re[0], rg[:, 0]
            outs = _run(mode, (acts, emb, G), rows)
            for i, (o, r) in enumerate(zip(outs, ref)):
                assert _mismatch(o, r) is None, (mode, rows, "point", p, "ranges of", sorted(pers), "output", i, _mismatch(o, r))
            acts[:, p], emb[p], G[:, p] = 0, blank, 0


# ---- (c) the raw task entry: dw_kernel with explicit ranges ----------------------------------------------------------------------------
RAW_CHUNKS = 40
RAW_LENS = (1, 2, 3, 4, 5, 8, 12, 13, 16, 17)
# variant -> (first column of A, M, leading dimension of B, first column of B, N): the operands sn_weight_grads gives that shape
RAW_GEOMETRY = {0: (0, 256, 256, 0, 256), 1: (0, 256, 128, 0, 64), 2: (0, 128, 256, 0, 256), 3: (0, 128, 128, 64, 64),
                4: (128, 32, 256, 0, 256), 5: (128, 32, 256, 0, 128)}


def _raw_formats(variant, flags):
    """storage of the (A, B) operand of a task: csrc/sn_dw_common.h `Task` -- 0x200: bf16 except the embedded inputs of variants 1 / 3;
    0x400: the 256-wide operands of variants 0 (a, b), 1 (a), 2 (b), 4 (b) are split rows, the rest fp32"""
    if flags == 0x300:
        return "bf16", ("f32" if variant in (1, 3) else "bf16")
    if flags == 0x500:
        return ("split" if variant in (0, 1) else "f32"), ("split" if variant in (0, 2, 4) else "f32")
    return "f32", "f32"


def _raw_operand(fmt, flags, values, col0, width, k0, k1):
    """(the operand array: NaN bytes everywhere but rows [k0, k1) x columns [col0, col0 + width) = `values`; the fp64 values consumed;
    the fp64 values stored)"""
    ld = values.shape[1]
    live = values[k0:k1, col0:col0 + width]
    if fmt == "split":
        assert col0 == 0 and width == ld == 256
        t = _nan_bytes((16 * RAW_CHUNKS, ld), torch.float32)
        t[k0:k1] = _x3_encode(live)
        return t, _x3_value(live), _x3_value(live)
    t = _nan_bytes((16 * RAW_CHUNKS, ld), torch.bfloat16 if fmt == "bf16" else torch.float32)
    t[k0:k1, col0:col0 + width] = live.to(t.dtype)
    stored = t[k0:k1, col0:col0 + width].double()
    consumed = stored if flags in (0, 0x500) else live.bfloat16().double()     # fp32 MFMAs / split in registers: the fp32 value itself
    return t, consumed, stored


@pytest.mark.parametrize("flags", [0, 0x100, 0x300, 0x500])
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
def test_raw_task_entry_ranges_vs_fp64(variant, flags):
    """(c) sn_dw_gemm, one task per range length of RAW_LENS chunks somewhere inside a 40-chunk operand (k0 != 0), every row outside the
    task's range and every column outside its tile NaN: the partial C and the partial bias of each task exactly 16 x chunks for all-ones
    operands, and within the bars of (a) of the fp64 contraction of its rows for random ones.  Measured worst C / bias over all variants
    and lengths: flags 0: 3.0e-07 / 1.4e-07, 0x100: 9.0e-08 / 6.4e-08, 0x300: 9.0e-08 / 2.1e-08, 0x500: 4.6e-06 / 8.3e-08."""
    a_col, M, ldb, b_col, N = RAW_GEOMETRY[variant]
    fa, fb = _raw_formats(variant, flags)
    g = torch.Generator(device=dev())
    g.manual_seed(100 * variant + flags)
    for kind in ("ones", "random"):
        keep, rows_, want = [], [], []
        for L in RAW_LENS:
            k0 = 16 * (1 + (7 * L) % (RAW_CHUNKS - L))
            k1 = k0 + 16 * L
            assert 0 < k0 < k1 <= 16 * RAW_CHUNKS
            if kind == "ones":
                va, vb = torch.ones((16 * RAW_CHUNKS, 256), device=dev()), torch.ones((16 * RAW_CHUNKS, ldb), device=dev())
            else:
                va = torch.randn((16 * RAW_CHUNKS, 256), device=dev(), generator=g) * 0.1 + 0.02
                vb = torch.randn((16 * RAW_CHUNKS, ldb), device=dev(), generator=g)
            ta, ca, sa = _raw_operand(fa, flags, va, a_col, M, k0, k1)
            tb, cb, _ = _raw_operand(fb, flags, vb, b_col, N, k0, k1)
            c = torch.full((M, N), NAN, device=dev())
            bias = torch.full((M,), NAN, device=dev())
            keep.append((ta, tb, c, bias))
            rows_.append((ta.data_ptr() + a_col * ta.element_size(), tb.data_ptr() + b_col * tb.element_size(), c.data_ptr(), bias.data_ptr(),
                          k0, k1, 256 | (ldb << 32), N | ((variant | flags) << 32)))
            want.append((ca.T @ cb, sa.sum(0)))
        tasks = torch.from_numpy(np.asarray(rows_, dtype=np.int64)).to(dev())
        _lib.check(_lib.lib.sn_dw_gemm(_lib.ptr(tasks), tasks.shape[0], None), "sn_dw_gemm")
        torch.cuda.synchronize()
        for L, (_, _, c, bias), (wc, wb) in zip(RAW_LENS, keep, want):
            at = ("variant", variant, "flags", hex(flags), kind, "chunks", L)
            assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(bias).all()), at
            if kind == "ones":
                assert bool((wc == 16.0 * L).all()) and bool((wb == 16.0 * L).all())
                assert _mismatch(c, wc.float()) is None, at + ("C", _mismatch(c, wc.float()))
                assert _mismatch(bias, wb.float()) is None, at + ("bias", _mismatch(bias, wb.float()))
            else:
                ec = ((c.double() - wc).norm() / wc.norm()).item()
                eb = ((bias.double() - wb).norm() / wb.norm()).item()
                print("dw-edges raw variant %d flags %#x chunks %d C %.3e bias %.3e" % (variant, flags, L, ec, eb))
                assert ec < (1e-5 if flags == 0 else 2e-5), at + (ec,)
                assert eb < 1e-5, at + (eb,)
