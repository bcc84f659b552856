"""The drop-in claim, exercised through the reference's OWN callers (VERDICT r3 "Next round" #3).

`eval.py::batched_inference` (eval.py:84-115) and `models/sinnerf.py::SinNeRF.forward` (sinnerf.py:171-193) are imported
UNMODIFIED from the staged reference tree (oracle/_ref, byte-for-byte, git-ignored; oracle/stage_ref.py) with stub modules for
the third-party packages this image lacks (cv2, torchvision, kornia, pytorch_lightning, imageio, piq), after
`models.rendering.render_rays` / `models.nerf.{NeRF, Embedding}` were replaced by `sinnerf_amd`'s exactly as INTEGRATION.md §1
prescribes.  Their output dicts are held to the numpy oracle at the fp32 bar on BASELINE config 1's shape (a 1 024-ray chunk of a
504x378 llff frame, white_back=False) and on a 4 096-ray lego batch (config 2's batch).

CPU half (no GPU needed): the same harness with NOTHING patched runs the reference's own path and must equal the oracle -- so a
green GPU test cannot be an artefact of the stubs.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import oracle_np as O          # noqa: E402
from oracle import stage_ref               # noqa: E402
from tests.helpers import check_render     # noqa: E402


def _callers(patch=None):
    if not stage_ref.callers_available():
        pytest.skip("oracle/_ref does not hold the reference callers (build() stages them where a checkout of the reference is present)")
    return stage_ref.load_callers(patch)


def _hparams(**kw):
    hp = dict(N_samples=64, N_importance=64, use_disp=False, perturb=0, noise_std=0, chunk=32 * 1024)
    hp.update(kw)
    return SimpleNamespace(**hp)


def _sinnerf_instance(sn, models, embeddings, hparams, white_back):
    """a SinNeRF object without its constructor (which opens datasets and downloads DINO weights): exactly the attributes
    SinNeRF.forward reads (sinnerf.py:171-186)"""
    obj = sn.SinNeRF.__new__(sn.SinNeRF)
    torch.nn.Module.__init__(obj)
    obj.hparams = hparams
    obj.models, obj.embeddings = models, embeddings
    obj.train_dataset = SimpleNamespace(white_back=white_back)
    return obj


def test_harness_runs_the_reference_callers_on_the_reference_path_cpu():
    ev, sn = _callers(None)
    assert ev.render_rays.__module__ == "models.rendering" and sn.render_rays is ev.render_rays
    params = [O.init_params(s, teacher=True) for s in (0, 1)]
    models, emb = [], [sn.Embedding(3, 10), sn.Embedding(3, 4)]
    for p in params:
        m = sn.NeRF(use_new_activation=True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
        models.append(m.eval())
    rays = O.llff_like_rays(96, seed=3)
    ref = O.render_rays(params, rays, 64, False, 0, 0, 64, 32768, False, False)
    torch.set_num_threads(4)
    ev.dataset = SimpleNamespace(white_back=False)                      # the module global batched_inference reads (eval.py:105)
    out = ev.batched_inference(models, emb, torch.from_numpy(rays), 64, 64, False, 32768, False)
    check_render({k: v.numpy() for k, v in out.items()}, ref, tag="ref batched_inference (cpu)")
    obj = _sinnerf_instance(sn, models, emb, _hparams(), white_back=False)
    with torch.no_grad():
        out2 = sn.SinNeRF.forward(obj, torch.from_numpy(rays))
    check_render({k: v.numpy() for k, v in out2.items()}, ref, tag="ref SinNeRF.forward (cpu)")


def _amd_models(dev, compute_dtype="fp32"):
    import sinnerf_amd
    params, models = [], []
    for s in (0, 1):
        p = O.init_params(s, teacher=True)
        m = sinnerf_amd.NeRF(use_new_activation=True, compute_dtype=compute_dtype)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
        models.append(m.to(dev).eval()); params.append(p)
    return params, models


@pytest.mark.gpu
def test_reference_eval_batched_inference_with_sinnerf_amd_patched_in():
    import sinnerf_amd
    dev = torch.device("cuda:0")
    ev, sn = _callers(sinnerf_amd)
    assert ev.render_rays is sinnerf_amd.render_rays and ev.NeRF is sinnerf_amd.NeRF and ev.Embedding is sinnerf_amd.Embedding
    params, models = _amd_models(dev)
    emb = [ev.Embedding(3, 10), ev.Embedding(3, 4)]                     # eval.py:134-135
    rays = O.llff_like_rays(1024, seed=5)                                # BASELINE configs[0]: one chunk of 1024 rays, llff 504x378
    ref = O.render_rays(params, rays, 64, False, 0, 0, 64, 32768, False, False)
    ev.dataset = SimpleNamespace(white_back=False)
    out = ev.batched_inference(models, emb, torch.from_numpy(rays).to(dev), 64, 64, False, 32768, False)
    assert set(out) == {"rgb_coarse", "depth_coarse", "opacity_coarse", "rgb_fine", "depth_fine", "opacity_fine"}
    check_render({k: v.cpu().numpy() for k, v in out.items()}, ref, tag="eval.batched_inference -> sinnerf_amd")


@pytest.mark.gpu
def test_reference_sinnerf_forward_with_sinnerf_amd_patched_in():
    import sinnerf_amd
    dev = torch.device("cuda:0")
    ev, sn = _callers(sinnerf_amd)
    assert sn.render_rays is sinnerf_amd.render_rays and sn.NeRF is sinnerf_amd.NeRF
    params, models = _amd_models(dev)
    emb = [sn.Embedding(3, 10), sn.Embedding(3, 4)]                     # sinnerf.py:133-134
    rays = np.ascontiguousarray(O.lego_rays(400, 400, seed=2)[::39][:4096])        # one 4096-ray lego batch (config 2)
    # chunk 1536 < 4096: the reference's ray-chunk loop + torch.cat (sinnerf.py:175-192) really iterates (3 chunks, ragged tail)
    obj = _sinnerf_instance(sn, models, emb, _hparams(chunk=1536), white_back=True)
    with torch.no_grad():
        out = sn.SinNeRF.forward(obj, torch.from_numpy(rays).to(dev))
    ref = O.render_rays(params, rays, 64, False, 0, 0, 64, 32768, True, False)
    check_render({k: v.cpu().numpy() for k, v in out.items()}, ref, tag="SinNeRF.forward -> sinnerf_amd")
    # training defaults (perturb=1, noise_std=1, opt.py:25-28) under autograd: the reference caller and this repo's mirror
    # (system.SinNeRFSystem.forward) consume the device RNG identically -> bit-identical results and gradients
    for m in models:
        m.train()
    obj.hparams = _hparams(perturb=1.0, noise_std=1.0)
    r = torch.from_numpy(rays).to(dev)
    torch.manual_seed(11)
    a = sn.SinNeRF.forward(obj, r)
    (a["rgb_fine"].sum() + a["depth_coarse"].sum()).backward()
    ga = [p.grad.clone() for m in models for p in m.parameters()]
    for m in models:
        m.zero_grad(set_to_none=True)
    from sinnerf_amd.system import SinNeRFSystem
    mirror = SinNeRFSystem(N_importance=64, perturb=1.0, noise_std=1.0, white_back=True)
    mirror.models, mirror.embeddings = models, emb
    torch.manual_seed(11)
    b = mirror(r)
    (b["rgb_fine"].sum() + b["depth_coarse"].sum()).backward()
    gb = [p.grad for m in models for p in m.parameters()]
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert all(torch.isfinite(x).all() for x in ga) and sum(float(x.abs().sum()) for x in ga) > 0
