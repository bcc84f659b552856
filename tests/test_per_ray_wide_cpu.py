"""CPU: the oracle side of the wide (more than 64 samples per ray) per-ray tests, and proof that their acceptance functions
reject a kernel with a wrong element-to-lane map -- shown on numpy restatements of the kernels, so it needs no GPU."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import per_ray_wide as W
from tests.helpers import GOLDEN, sample_pdf_tol, well_conditioned


def test_linspace_matches_torch_every_n():
    torch = pytest.importorskip("torch")
    for n in range(1, 1101):
        assert np.array_equal(O.linspace01(n), torch.linspace(0, 1, n).numpy()), n


@pytest.mark.parametrize("m,k", [(300, 257), (1000, 64)])
def test_sample_pdf_wide_fixture(m, k):
    """the assertions of test_oracle_golden.test_sample_pdf on sample_pdf_wide.npz (reference outputs at 300 and 1000 bins)"""
    z = np.load(f"{GOLDEN}/sample_pdf_wide.npz")
    bins, w, u = z[f"m{m}_bins"], z[f"m{m}_weights"], z[f"m{m}_u"]
    assert w.shape == (24, m) and u.shape == (24, k)
    det = O.sample_pdf(bins, w, k, det=True)
    rnd = O.sample_pdf(bins, w, k, det=False, u=u)
    lin = O.linspace01(k)[None].repeat(24, 0)
    ok_det, ok_rnd = well_conditioned(bins, w, lin), well_conditioned(bins, w, u)
    assert ok_det.mean() > 0.97 and ok_rnd.mean() > 0.97
    assert (np.abs(det - z[f"m{m}_out_det"]) <= sample_pdf_tol(bins, w, lin))[ok_det].all()
    assert (np.abs(rnd - z[f"m{m}_out_rand"]) <= sample_pdf_tol(bins, w, u))[ok_rnd].all()
    assert (det >= bins[:, :1] - 1e-6).all() and (det <= bins[:, -1:] + 1e-6).all()


def test_shapes_reach_the_chunk_sizes_they_name():
    for S, _, _ in W.SAMPLER_SHAPES:
        assert W.chunk(S - 2) == W.SAMPLER_C[S], S
    assert sorted({W.chunk(S) for S in W.COMPOSITE_BWD_S}) == [2, 4, 5, 9, 11, 16]
    assert sorted({W.chunk(S) for S in W.COMPOSITE_FWD_S}) == [2, 5, 9, 15, 16]
    assert W.lane_boundaries(130)[:5] == [2, 3, 5, 6, 8] and W.lane_boundaries(130)[-1] == 129
    assert W.lane_boundaries(1024)[:4] == [15, 16, 31, 32] and len(W.lane_boundaries(1024)) == 127


@pytest.mark.parametrize("S,NI,family,rand_u", W.SAMPLER_CASES)
def test_sampler_acceptance_passes_the_kernel_arithmetic_and_rejects_a_strided_scan(S, NI, family, rand_u):
    zc, w, u = W.sampler_inputs(S, NI, family, rand_u)
    tag = f"S{S}_NI{NI}_{family}_{'rand' if rand_u else 'det'}"
    worst, share = W.check_sampler(zc, w, u, NI, *W.emulate_sampler(zc, w, u, NI), tag=tag)
    print(tag, "emulation err/tol %.3f, well-conditioned share %.4f" % (worst, share))
    with pytest.raises(AssertionError):                     # every shape here has C > 1
        W.check_sampler(zc, w, u, NI, *W.emulate_sampler(zc, w, u, NI, strided=True), tag=tag + "_strided")


@pytest.mark.parametrize("S", W.COMPOSITE_BWD_S)
def test_backward_bar_passes_the_kernel_arithmetic_and_rejects_a_forgotten_carry(S):
    rays, z, raw, noise, r = W.composite_inputs(S, 9, 2)
    n = rays.shape[0]
    white_back, noise_std, with_gw = W.backward_settings(S)
    g_rgb, g_depth = r.standard_normal((n, 3)).astype(np.float32), r.standard_normal(n).astype(np.float32)
    g_w = r.standard_normal((n, S)).astype(np.float32) if with_gw else None
    args = (raw, z, rays[:, 3:6], noise if noise_std else None, noise_std, white_back, g_rgb, g_depth, g_w)
    ref = O.composite_backward(*args)
    worst = W.check_backward(W.emulate_composite_backward(*args), ref, f"S{S}")
    print(f"S{S}: emulation err/bar {worst:.3f}")
    used = -(-S // W.chunk(S))                              # lanes that hold samples
    for b in (0, used // 2, used - 2):                      # one forgotten carry, at the first, a middle and the last boundary
        with pytest.raises(AssertionError):
            W.check_backward(W.emulate_composite_backward(*args, forget_carry_at=b), ref, f"S{S}_forget{b}")


@pytest.mark.parametrize("S", W.COMPOSITE_BWD_S)
def test_backward_probe_reference_and_sensitivity(S):
    """the closed form of the position probe equals the oracle's backward for the same upstream gradient, the kernel arithmetic
    passes it, and a carry forgotten at any lane boundary leaves the bar"""
    rays, z, raw, g_w, j = W.probe_inputs(S)
    n = rays.shape[0]
    assert list(j) == W.lane_boundaries(S)
    zero3, zero1 = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    ref = W.probe_reference(rays, z, raw, j)
    orc = O.composite_backward(raw, z, rays[:, 3:6], None, 0.0, False, zero3, zero1, g_w)
    assert np.abs(ref - orc).max() <= 1e-12 * np.abs(ref).max()
    args = (raw, z, rays[:, 3:6], None, 0.0, False, zero3, zero1, g_w)
    W.check_backward(W.emulate_composite_backward(*args), ref, f"probe_S{S}")
    used = -(-S // W.chunk(S))
    for b in (0, used // 3, used // 2, used - 2):
        with pytest.raises(AssertionError):
            W.check_backward(W.emulate_composite_backward(*args, forget_carry_at=b), ref, f"probe_S{S}_forget{b}")
