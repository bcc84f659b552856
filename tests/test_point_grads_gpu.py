"""GPU: ``sn_point_grads`` and ``sn_point_grads_wsum`` against float64 restatements (tests/point_grad_oracle.py, pinned to the reference
by tests/test_point_grads_cpu.py) on synthetic pre-activation gradients: every state layout, pad rows that must never be read, pad
lanes that must never write, one embedding column at a time, bit-repeatability."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import point_grad_oracle as PG                                                # noqa: E402
from tests.helpers import x3_state_decode, x3_state_encode                               # noqa: E402
from tests.test_parity_gpu import dev                                                    # noqa: E402
from tests.test_ray_grads_gpu import make_inputs, t, weights3                            # noqa: E402

# |got - ref| <= BOUND * A per component, A = the same computation with every factor replaced by its absolute value: the bound of
# tests/test_ray_grads_gpu.py without the sum over samples -- 512 k steps + 21 embedding terms in fp32 -> 533 * 2^-24 = 3.2e-5
BOUND = 5e-5
SHAPES = [(1, 1), (5, 37), (3, 192), (2, 1024)]          # one point; a partial wave tile; > one 256-point tile, partial last; widest ray
GUARD = 64                                               # rows behind the output that must stay untouched


def call_point_grads(w1, w5, G, code, rays, z):
    """sn_point_grads through ctypes: numpy weights / rays / z, G = device tensor in the layout `code` names -> (P, 4) numpy"""
    from sinnerf_amd import _lib as L
    n, S = z.shape
    P = n * S
    out = torch.full((P + GUARD, 4), float("nan"), dtype=torch.float32, device=dev())
    w1t, w5t, rt, zt = t(w1, torch.float32), t(w5, torch.float32), t(rays), t(z)
    L.check(L.lib.sn_point_grads(L.ptr(w1t), L.ptr(w5t), code, L.ptr(G), G.shape[1], L.ptr(rt), L.ptr(zt), n, S, L.ptr(out),
                                 L.stream_ptr()), "sn_point_grads")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[P:]).all(), "a pad lane stored behind the last point"
    return got[:P]


def call_wsum(g_xyz, w):
    from sinnerf_amd import _lib as L
    n, S = w.shape
    out = torch.full((n + GUARD, 4), float("nan"), dtype=torch.float32, device=dev())
    gt, wt = t(g_xyz), t(w)
    L.check(L.lib.sn_point_grads_wsum(L.ptr(gt), L.ptr(wt), n, S, L.ptr(out), L.stream_ptr()), "sn_point_grads_wsum")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[n:]).all()
    return got[:n]


def check_bound(got, ref, A, tag):
    """got (P, 4) fp32 against ref / A (n, S, 3) float64"""
    assert np.isfinite(got).all(), tag
    assert (got[:, 3] == 0).all(), tag
    ref, A = ref.reshape(-1, 3), A.reshape(-1, 3)
    worst = float((np.abs(got[:, :3] - ref) / (BOUND * A + 1e-300)).max())
    print(tag, "max err / (5e-5 A) =", worst)
    assert worst <= 1.0, (tag, worst)


def check_wsum(got, g_xyz, w, tag):
    """|g_sum - sum64| <= 2^-24 |sum64| + S 2^-52 sum |w g|: fp64 products of fp32 values are exact, S fp64 additions, ONE rounding to fp32"""
    n, S = w.shape
    prod = w.astype(np.float64)[:, :, None] * g_xyz.reshape(n, S, 4)[:, :, :3].astype(np.float64)
    ref, mag = prod.sum(1), np.abs(prod).sum(1)
    assert np.isfinite(got).all() and (got[:, 3] == 0).all(), tag
    err = np.abs(got[:, :3].astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + S * 2.0 ** -52 * mag
    assert (err <= bound).all(), (tag, float((err / (bound + 1e-300)).max()))


@pytest.mark.parametrize("n,S", SHAPES)
def test_point_grads_dense_vs_float64(n, S):
    from sinnerf_amd import _lib as L
    w1, w5, _ = weights3()
    rays, z, G, P = make_inputs(n, S, 200 + S)
    Gt = t(G)                                                                             # pad rows NaN: they must never be read
    got = call_point_grads(w1, w5, Gt, L.SN_DTYPE_F32, rays, z)
    ref = PG.point_grads_mlp(G[0, :P], G[4, :P], w1, w5, rays, z)
    A = PG.point_grads_mlp(G[0, :P], G[4, :P], w1, w5, rays, z, abs_bound=True)
    check_bound(got, ref, A, f"dense ({n},{S})")
    again = call_point_grads(w1, w5, Gt, L.SN_DTYPE_F32, rays, z)
    assert got.tobytes() == again.tobytes()                                               # no atomics, fixed order
    assert got.tobytes() == call_point_grads(w1, w5, Gt, L.SN_DTYPE_BF16, rays, z).tobytes()   # fp32 state, bf16-operand chain
    # the weighted sum over each ray's samples, from the kernel's own output
    r = np.random.RandomState(S)
    w = r.uniform(0, 1, (n, S)).astype(np.float32)
    w[r.uniform(0, 1, (n, S)) < 0.3] = 0.0                                                # compositing weights are often exactly zero
    gs = call_wsum(got, w)
    check_wsum(gs, got, w, f"wsum ({n},{S})")
    assert gs.tobytes() == call_wsum(got, w).tobytes()


@pytest.mark.parametrize("n,S", [(1, 1), (5, 63), (6, 64), (9, 65), (3, 1024)])
def test_point_grads_wsum_wide_range(n, S):
    """signed weights and gradients over 12 decades, more rays than one block holds (4), sample counts around the wave width"""
    r = np.random.RandomState(1000 + S)
    g = (r.standard_normal((n * S, 4)) * 10.0 ** r.uniform(-6, 6, (n * S, 1))).astype(np.float32)
    g[:, 3] = np.nan                                                                      # the fourth column is not an input
    w = r.standard_normal((n, S)).astype(np.float32)
    check_wsum(call_wsum(g, w), g, w, f"wsum wide ({n},{S})")


def test_point_grads_one_embedding_column_at_a_time():
    """A / |ref| of the dense test is large (the 2^9 band dominates): a wrong identity or low-band column would hide there.
    One-hot weights isolate column order, band scale and the sin / cos sign of every column."""
    from sinnerf_amd import _lib as L
    n, S = 5, 37
    rays, z, G, P = make_inputs(n, S, 7)
    xyz_cols = [0, 1, 2, 3, 5, 6, 8, 27, 31, 33, 38, 57, 59, 60, 62]
    for which, slot in (("w1", 0), ("w5", 4)):
        Gs = np.zeros_like(G)
        Gs[:, P:] = np.nan
        Gs[slot, :P, 0] = G[slot, :P, 0]
        Gt = t(Gs)
        for c in xyz_cols:
            w1, w5 = np.zeros((256, 63), np.float32), np.zeros((256, 319), np.float32)
            {"w1": w1, "w5": w5}[which][0, c] = 1.0
            got = call_point_grads(w1, w5, Gt, L.SN_DTYPE_F32, rays, z)
            ref = PG.point_grads_mlp(Gs[0, :P], Gs[4, :P], w1, w5, rays, z).reshape(-1, 3)
            A = PG.point_grads_mlp(Gs[0, :P], Gs[4, :P], w1, w5, rays, z, abs_bound=True).reshape(-1, 3)
            assert np.abs(ref).max() > 0
            assert np.isfinite(got).all() and (got[:, 3] == 0).all()
            err = np.abs(got[:, :3] - ref)
            assert (err <= BOUND * A).all(), (which, c, float((err / (BOUND * A + 1e-300)).max()))
    # a column of xyz_encoding_5 behind the 63 embedded inputs (the h4 block of the skip) must not reach the result
    w1, w5 = np.zeros((256, 63), np.float32), np.zeros((256, 319), np.float32)
    w5[:, 63:] = 1.0
    assert (call_point_grads(w1, w5, t(G), L.SN_DTYPE_F32, rays, z) == 0).all()


def test_point_grads_state_layouts():
    """the same values stored as bf16 rows / as the (hi, lo) pairs of the bf16x3 state; reference from the DECODED values"""
    from sinnerf_amd import _lib as L
    w1, w5, _ = weights3()
    for n, S in ((5, 37), (3, 192)):
        rays, z, G, P = make_inputs(n, S, 11 + S)
        # bf16 rows
        G16 = t(G).to(torch.bfloat16)
        dec = G16.float().cpu().numpy()
        got = call_point_grads(w1, w5, G16, L.SN_DTYPE_BF16_STATE, rays, z)
        args = (dec[0, :P], dec[4, :P], w1, w5, rays, z)
        check_bound(got, PG.point_grads_mlp(*args), PG.point_grads_mlp(*args, abs_bound=True), f"bf16 rows ({n},{S})")
        # bf16x3 state: slots 0..8 as (hi, lo) pairs
        fin = np.where(np.isfinite(G), G, 0.0).astype(np.float32)
        Gx = np.array(G, copy=True)
        Gx[:9] = x3_state_encode(fin[:9])
        dec = x3_state_decode(Gx[:9])
        Gx[:, P:] = np.nan
        Gx[:9, P:] = np.full(1, 0x7FC07FC0, np.uint32).view(np.float32)[0]                # two bf16 NaNs per word in the pad rows
        got = call_point_grads(w1, w5, t(Gx), L.SN_DTYPE_BF16X3, rays, z)
        args = (dec[0, :P], dec[4, :P], w1, w5, rays, z)
        check_bound(got, PG.point_grads_mlp(*args), PG.point_grads_mlp(*args, abs_bound=True), f"bf16x3 state ({n},{S})")
        assert got.tobytes() == call_point_grads(w1, w5, t(Gx), L.SN_DTYPE_BF16X3, rays, z).tobytes()
    # anything else, flag bits included, is refused
    for code in (L.SN_DTYPE_F16, L.SN_DTYPE_F32 | L.SN_DTYPE_CLASSIC_HEADS, L.SN_DTYPE_BF16_STATE | L.SN_DTYPE_EMB_BF16,
                 L.SN_DTYPE_BF16X3 | L.SN_DTYPE_COMPILER_SCHEDULED, 7):
        with pytest.raises(L.SinnerfHipError):
            call_point_grads(w1, w5, t(G), code, rays, z)
