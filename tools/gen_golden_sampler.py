#!/usr/bin/env python3
"""One golden training sample of the reference's one-image dataset, from the UNMODIFIED reference (run in the build container only, like
tools/gen_golden_warp.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_sampler.py

The dataset module needs cv2, torchvision and files on disk and cannot be imported whole: the ``__getitem__`` node of
``Blender_ray_patch_1image_rot3d_Dataset`` and the function nodes it calls (``rot_*``, ``rotate_3d``, ``convert``,
``project_with_depth``, ``forward_warp``, ``flatten``; ``create_meshgrid`` / ``get_ray_directions`` / ``get_rays`` of ``ray_utils.py``)
are compiled out of the mounted files (ast) at generation time; nothing of them is re-typed here.  ``__getitem__`` runs its train
branch on a stub object that carries the attributes the branch reads, with an ``np`` whose ``random`` records every ``randint`` /
``choice`` / ``normal`` result, and with ``forward_warp`` and ``get_rays`` wrapped to record what they return.

The scene: 40 x 40, a shaded disc with depth on a white, zero-depth background; ``patch_size = 8``, ``sW = sH = 2``, ``angle = 30``.

``tests/golden/sampler.npz`` holds:

    H, W, patch_size, sW, sH, angle, near, far, focal       the settings
    rgb (H, W, 3), depth (H, W), c2w (4, 4), K (3, 3)       the inputs, fp32
    all_rays (H W, 8)                                       the stub's ray table of the reference pose (the reference's get_rays)
    side_c2w (3, 4), side_rays (H W, 8)                     the pose __getitem__ drew and the rays its get_rays returned for it, with the
                                                            near / far columns of the table
    warp_out (H, W, 3), warp_depth (H, W)                   what its forward_warp returned (full frame)
    draw_log                                                the calls of np.random in order, as text: "randint 25 -> 7" ...
    real_ll, real_up, side_ll, side_up                      the origins the two loops accepted;  real_tries, side_tries: how often they drew
    ray_idx, ray_idx2, ray_idx_proj, angles                 the other draws
    sample_<key>                                            every tensor of the returned sample
"""
import ast
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SINNERF_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "sampler.npz")
HELPERS = ("rot_phi", "rot_theta", "rot_z", "rotate_3d", "convert", "project_with_depth", "forward_warp", "flatten")
RAY_HELPERS = ("create_meshgrid", "get_ray_directions", "get_rays")
H = W = 40
PS, SW, SH, ANGLE, NEAR, FAR, SEED = 8, 2, 2, 30, 2.0, 6.0, 3


class RandomSpy:
    """np.random, with the results of randint / choice / normal recorded in call order"""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        return getattr(np.random, name)

    def _record(self, name, args, result):
        self.log.append((name, args, np.array(result)))
        return result

    def randint(self, *args, **kw):
        return self._record("randint", args, np.random.randint(*args, **kw))

    def choice(self, *args, **kw):
        return self._record("choice", args, np.random.choice(*args, **kw))

    def normal(self, *args, **kw):
        return self._record("normal", args, np.random.normal(*args, **kw))


class NpSpy:
    def __init__(self):
        self.random = RandomSpy()

    def __getattr__(self, name):
        return getattr(np, name)


def recording(fn, into):
    def wrapped(*args, **kw):
        out = fn(*args, **kw)
        into.append(out)
        return out
    return wrapped


def compile_reference(np_module):
    """namespace with the reference's own nodes: the ray helpers, the warp helpers and the dataset's __getitem__ as a plain function"""
    ns = {"torch": torch, "np": np_module}
    path = os.path.join(REF, "datasets", "ray_utils.py")
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in RAY_HELPERS]
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    path = os.path.join(REF, "datasets", "blender_ray_patch_1image_rot3d.py")
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in HELPERS]
    for cls in tree.body:
        if isinstance(cls, ast.ClassDef) and cls.name == "Blender_ray_patch_1image_rot3d_Dataset":
            nodes += [m for m in cls.body if isinstance(m, ast.FunctionDef) and m.name == "__getitem__"]
    assert [n.name for n in nodes][-1] == "__getitem__"
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns


def scene():
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r2 = (x - 19.5) ** 2 + (y - 19.5) ** 2
    disc = r2 < 12.0 ** 2
    shade = np.stack([0.5 + 0.4 * np.sin(0.37 * x), 0.5 + 0.4 * np.cos(0.23 * y), 0.7 + 0.0 * x], -1)
    rgb = np.where(disc[..., None], shade, 1.0).astype(np.float32)
    depth = np.where(disc, 4.0 - 0.05 * np.sqrt(np.maximum(144.0 - r2, 0.0)), 0.0).astype(np.float32)
    return rgb, depth


def stub(ns, rgb, depth, c2w, focal):
    """the attributes the train branch of __getitem__ reads, built as the dataset's __init__ builds them, with the reference's helpers"""
    s = types.SimpleNamespace()
    s.split, s.patch_size, s.sW, s.sH, s.angle, s.near, s.far, s.load_depth = "train", PS, SW, SH, ANGLE, NEAR, FAR, True
    img = torch.from_numpy(rgb).permute(2, 0, 1).contiguous()
    s.imgs_2d, s.img_num = [img], 1
    s.ref_view, s.ref_depth, s.ref_c2w = img.permute(1, 2, 0), torch.from_numpy(depth), torch.from_numpy(c2w)
    s.K = torch.tensor([[focal, 0, (W - 1) / 2], [0, focal, (H - 1) / 2], [0, 0, 1]], dtype=torch.float32)
    s.directions = ns["get_ray_directions"](H, W, focal)
    rays_o, rays_d = ns["get_rays"](s.directions, s.ref_c2w[:3, :4])
    rays = torch.cat([rays_o, rays_d, NEAR * torch.ones_like(rays_o[:, :1]), FAR * torch.ones_like(rays_o[:, :1])], 1)
    s.all_rays, s.all_rgbs, s.all_depth = rays, img.view(3, -1).permute(1, 0), s.ref_depth.reshape(-1, 1)
    nonwhite = s.all_rgbs.sum(-1) != 3
    s.nonzero_rays, s.nonzero_rgbs, s.nonzero_depth = rays[nonwhite], s.all_rgbs[nonwhite], s.all_depth[nonwhite]
    s.rgb_num, s.all_rgb_num = int(nonwhite.sum()), H * W
    s.ref_rays = rays.view(W, H, 8)
    # the table of pre-warped poses is not part of the fixture: its slots only need to exist
    s.proj_rays_full, s.proj_depths_full, s.proj_mat, s.ref_proj_mat = rays, s.all_depth, [torch.eye(4)], torch.eye(4)
    s.poses_real, s.poses_fake, s.len_full = torch.zeros(16), [torch.zeros(12)], 1
    return s


def accepted_origins(log):
    """(real_ll, real_up, real_tries, side_ll, side_up, side_tries) from the call log: randint #0 is new_idx; pairs up to the first choice
    belong to the real loop, the pairs after the normals to the unseen-view loop"""
    names = [e[0] for e in log]
    first_choice, last_normal = names.index("choice"), len(names) - 1 - names[::-1].index("normal")
    real = [int(e[2]) for e in log[1:first_choice]]
    side = [int(e[2]) for e in log[last_normal + 1:] if e[0] == "randint"]
    assert names[0] == "randint" and len(real) % 2 == 0 and len(side) % 2 == 0 and real and side
    return real[-2], real[-1], len(real) // 2, side[-2], side[-1], len(side) // 2


def main():
    spy = NpSpy()
    ns = compile_reference(spy)
    warps, rays_of = [], []
    rgb, depth = scene()
    c2w = np.eye(4, dtype=np.float32)
    c2w[2, 3] = 4.0
    focal = float(0.5 * W / np.tan(0.5 * 0.69))
    s = stub(ns, rgb, depth, c2w, focal)                  # before the wrappers: the stub's own get_rays call is not recorded
    ns["forward_warp"] = recording(ns["forward_warp"], warps)
    ns["get_rays"] = recording(ns["get_rays"], rays_of)
    np.random.seed(SEED)
    sample = ns["__getitem__"](s, 0)
    log = spy.random.log
    assert len(warps) == 1 and len(rays_of) == 1
    rays_o, rays_d = rays_of[0]
    side_rays = torch.cat([rays_o, rays_d, NEAR * torch.ones_like(rays_o[:, :1]), FAR * torch.ones_like(rays_o[:, :1])], 1)
    choices = [e[2] for e in log if e[0] == "choice"]
    angles = np.array([float(e[2]) for e in log if e[0] == "normal"])
    real_ll, real_up, real_tries, side_ll, side_up, side_tries = accepted_origins(log)
    assert len(choices) == 3 and angles.shape == (3,)
    side_c2w = ns["rotate_3d"](s.ref_c2w, *angles)
    arrays = dict(H=H, W=W, patch_size=PS, sW=SW, sH=SH, angle=ANGLE, near=NEAR, far=FAR, focal=focal, rgb=rgb, depth=depth, c2w=c2w,
                  K=s.K.numpy(), all_rays=s.all_rays.numpy(), side_c2w=torch.FloatTensor(side_c2w)[:3, :4].numpy(),
                  side_rays=side_rays.numpy(), warp_out=np.asarray(warps[0][0], np.float32), warp_depth=np.asarray(warps[0][1], np.float32),
                  draw_log=np.array([f"{n} {' '.join(str(a) for a in args)} -> {r.tolist() if r.size <= 3 else '(%d values)' % r.size}"
                                     for n, args, r in log]),
                  real_ll=real_ll, real_up=real_up, real_tries=real_tries, side_ll=side_ll, side_up=side_up, side_tries=side_tries,
                  ray_idx=choices[0], ray_idx2=choices[1], ray_idx_proj=choices[2], angles=angles)
    for k, v in sample.items():
        if torch.is_tensor(v):
            arrays["sample_" + k] = v.numpy()
    np.savez_compressed(OUT, **arrays)
    print(f"real origin (ll, up) = ({real_ll}, {real_up}) after {real_tries} draw(s); unseen origin ({side_ll}, {side_up}) after "
          f"{side_tries}; angles {angles}; non-white {s.rgb_num}; landed {int((arrays['warp_depth'] != 0).sum())}")
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(arrays), "arrays")


if __name__ == "__main__":
    main()
