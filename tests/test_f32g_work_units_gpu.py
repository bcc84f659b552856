"""GPU: the fp32 inference kernel (csrc/sn_mlp_fwd_f32g.hip) deals 32-point work units to its waves by tickets drawn from a device word,
takes the ray index of a point from one scalar multiplication per unit plus a per-lane carry (csrc/sn_ray_index.h) and computes the
direction embedding once per wave where the wave's 32 points lie on one ray.  None of it may change a bit: every case below compares
against the LDS-ring kernel (SN_FLAG_F32_LDS_RING), which has a static tile loop, divides per lane and embeds per lane.  The shapes are
the smallest at which each new path can go wrong: a single point, fewer than 32 points, 32 k + 1 points, fewer units than a workgroup
has waves / than the chip has CUs, more units than the chip has waves (a wave draws a second ticket), rays shorter than a unit (the carry
is a division), rays that end inside a unit (S = 33, 37, 43: the mixed-ray fallback of the direction embedding) and rays that hold whole
units (S = 64, 128, 192, 1024: the shared embedding).  The formula of the ray index alone: tests/test_ray_index_cpu.py."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle_np as O                                          # noqa: E402
from tests.test_parity_gpu import dev                                      # noqa: E402

SHAPES = [(1, 1), (1, 31), (2, 33), (3, 37), (5, 64), (3, 128), (2, 192), (1, 1024),     # the issue's list
          (1, 33), (3, 43), (7, 5), (301, 3), (300, 128)]                                # 32 k + 1 points; short rays; 1 200 units


@functools.lru_cache(maxsize=None)
def _model(new_act):
    import sinnerf_amd
    m = sinnerf_amd.NeRF(use_new_activation=new_act)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in O.trained_params("fine").items()})
    return m.to(dev()).eval()


@functools.lru_cache(maxsize=None)
def _inputs(n, S):
    rays = O.lego_rays(400, 400, seed=3)
    rays = np.ascontiguousarray(rays[np.random.RandomState(n).choice(rays.shape[0], n, replace=False)])
    z = np.sort(np.random.RandomState(S).uniform(2, 6, (n, S)).astype(np.float32), -1)
    return torch.from_numpy(rays).to(dev()), torch.from_numpy(z).to(dev())


def _mlp(model, rays_t, z_t, sigma_only, flags):
    from sinnerf_amd import rendering
    with torch.no_grad():
        return rendering._mlp(model, rays_t, z_t, sigma_only, flags)


@pytest.mark.parametrize("n,S", SHAPES)
@pytest.mark.parametrize("sigma_only", [False, True])
@pytest.mark.parametrize("new_act", [True, False])
def test_work_units_ray_index_and_shared_embedding_keep_the_bits(n, S, sigma_only, new_act):
    from sinnerf_amd import _lib
    m = _model(new_act)
    rays_t, z_t = _inputs(n, S)
    a = _mlp(m, rays_t, z_t, sigma_only, 0)
    b = _mlp(m, rays_t, z_t, sigma_only, _lib.SN_FLAG_F32_LDS_RING)
    assert torch.isfinite(a).all() and torch.equal(a, b), (n, S, sigma_only, new_act)


@pytest.mark.parametrize("rows", [33, 129])
@pytest.mark.parametrize("new_act", [True, False])
def test_pre_embedded_rows_keep_the_bits(rows, new_act):
    """NeRF.forward under no_grad (pre-embedded rows, leading dimension 90) against the LDS-ring kernel on the same rows"""
    from sinnerf_amd import _lib
    m = _model(new_act)
    x = torch.from_numpy(np.random.RandomState(rows).standard_normal((rows, 90)).astype(np.float32)).to(dev())
    with torch.no_grad():
        a = m(x)
    b = torch.empty(rows, 4, device=dev())
    _lib.check(_lib.lib.sn_mlp_forward_embedded(_lib.ptr(m.packed()), m.kernel_dtype(), _lib.ptr(x), rows, 90, 0, _lib.SN_FLAG_F32_LDS_RING,
                                                _lib.ptr(b), _lib.stream_ptr()), "sn_mlp_forward_embedded")
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("n,S", [(3, 37), (300, 128)])
def test_repeated_launches_and_two_streams_give_the_same_result(n, S):
    """the ticket word is zeroed on the launch stream before every launch, and two streams never share a word: the same launch twice on
    one stream, then on two streams back to back (nothing orders the two against each other), all equal to the LDS-ring kernel's result"""
    from sinnerf_amd import _lib
    m = _model(True)
    rays_t, z_t = _inputs(n, S)
    ref = _mlp(m, rays_t, z_t, False, _lib.SN_FLAG_F32_LDS_RING)
    first, second = _mlp(m, rays_t, z_t, False, 0), _mlp(m, rays_t, z_t, False, 0)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(2):
        for s in (s1, s2):
            with torch.cuda.stream(s):
                outs.append(_mlp(m, rays_t, z_t, False, 0))
    torch.cuda.synchronize()
    for o in [first, second] + outs:
        assert torch.equal(o, ref)
