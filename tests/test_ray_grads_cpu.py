"""CPU: the pose-gradient entries exist in the library and the binding, and the float64 helper the GPU tests compare against
(tests/ray_grad_oracle.py) reproduces the ray gradients of the reference's own autograd (tools/gen_ray_grad_golden.py)."""
import numpy as np

from oracle import oracle_np as O
from tests import ray_grad_oracle as R
from tests.helpers import GOLDEN

NEW_SYMBOLS = ("sn_ray_grads_workspace_bytes", "sn_ray_grads", "sn_composite_backward_rays",
               "sn_generate_rays_backward_workspace_bytes", "sn_generate_rays_backward")


def load_ray_case(name):
    z = np.load(f"{GOLDEN}/{name}.npz")
    meta = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    rng = {k[4:]: z[k] for k in z.files if k.startswith("rng_")}
    coef = {k[5:]: z[k] for k in z.files if k.startswith("coef_")}
    return z, meta, rng, coef


def test_new_symbols_exported_within_abi_5():
    from sinnerf_amd import _lib as L
    assert L.lib.sn_abi_version() == L.ABI_VERSION == 5
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES, name
        assert getattr(L.lib, name) is not None
    assert L.lib.sn_ray_grads_workspace_bytes(5, 37) == 5 * 37 * 8 * 4
    assert L.lib.sn_ray_grads_workspace_bytes(5, 1025) == -5 and L.lib.sn_ray_grads_workspace_bytes(5, 0) == -5
    assert L.lib.sn_generate_rays_backward_workspace_bytes() > 0
    # argument checks run on the host before anything is launched
    assert L.lib.sn_ray_grads(None, None, None, 0, None, 0, None, None, 1, 1, None, None, None) == -1


def test_helper_reproduces_reference_ray_gradients():
    """The helper is pinned to the reference (never to the product): per pass nerf_forward -> composite_backward ->
    nerf_backward(gy_out) -> the formulas, against the reference's autograd on grad_rays_lego_det, to 3x the reference's own
    fp32-vs-fp64 spread on these inputs."""
    z, meta, rng, coef = load_ray_case("grad_rays_lego_det")
    models = [O.init_params(meta["seed_coarse"], True), O.init_params(meta["seed_fine"], True)]
    g_o, g_d = R.render_rays_ray_grads(models, z["rays"], coef, meta["N_samples"], meta["perturb"], meta["noise_std"],
                                       meta["N_importance"], bool(meta["white_back"]), rng)
    e_o, e_d = R.norm_err(g_o, z["g_o64"]), R.norm_err(g_d, z["g_d64"])
    print("helper vs reference float64: g_o", e_o, "g_d", e_d, "| spreads", float(z["spread_o"]), float(z["spread_d"]))
    assert e_o <= 3 * float(z["spread_o"]) and e_d <= 3 * float(z["spread_d"]), (e_o, e_d)
    e_o, e_d = R.norm_err(g_o, z["g_o"]), R.norm_err(g_d, z["g_d"])
    assert e_o <= 3 * float(z["spread_o"]) and e_d <= 3 * float(z["spread_d"]), (e_o, e_d)


def test_abs_bound_dominates():
    r = np.random.RandomState(0)
    n, S = 3, 5
    rays = O.lego_rays(20, 20, seed=1)[:n]
    zz = np.sort(r.uniform(2, 6, (n, S)).astype(np.float32), -1)
    G0, G4, G9 = (r.standard_normal((n * S, 256)) for _ in range(3))
    w1, w5, wd = r.standard_normal((256, 63)), r.standard_normal((256, 319)), r.standard_normal((128, 283))
    ref = R.ray_grads_mlp(G0, G4, G9, w1, w5, wd, rays, zz)
    A = R.ray_grads_mlp(G0, G4, G9, w1, w5, wd, rays, zz, abs_bound=True)
    assert (np.abs(ref) <= A).all() and (A[:, 6:] == 0).all() and (A[:, :6] > 0).all()
