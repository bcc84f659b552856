#!/usr/bin/env python3
"""When do the waves of the fp32 inference kernel run out of work?  Needs a -DSN_F32G_STAMP_EXIT build of csrc/sn_mlp_fwd_f32g.hip
(tools/build_variant_f32g.sh; every wave records s_memrealtime at entry and exit, its XCD and the units it drew) loaded through
SINNERF_HIP_LIB.  Runs the fine-pass (160 000 x 128) and the coarse-pass (160 000 x 64) launches of the bench and prints, as fractions
of the launch (first entry .. last exit): latest exit - mean exit and latest - earliest exit, over waves, workgroups (a workgroup ends
with its last wave) and XCDs (an XCD ends with its last workgroup).  What a kernel without a barrier loses to an uneven end is
`latest - mean`: the matrix time the average CU spends idle.
usage: SINNERF_HIP_LIB=build/variants/lib_f32g_<name>.so python tools/f32g_exit_spread.py [reps]"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle_np as O                      # noqa: E402  (input generator only)
import sinnerf_amd                                     # noqa: E402
from sinnerf_amd import rendering, _lib                # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
dev = torch.device("cuda:0")
set_buffer = _lib.lib.sn_f32g_set_stamp_buffer         # AttributeError: not a stamp build
set_buffer.restype, set_buffer.argtypes = None, [ctypes.c_void_p]
n_wg = torch.cuda.get_device_properties(0).multi_processor_count
stamps = torch.zeros((n_wg * 4, 4), dtype=torch.int64, device=dev)
set_buffer(ctypes.c_void_p(stamps.data_ptr()))

rays = torch.from_numpy(O.lego_rays(400, 400, 0)).to(dev)
m = sinnerf_amd.NeRF(use_new_activation=True, compute_dtype="fp32")
m.load_state_dict({k: torch.from_numpy(v) for k, v in O.init_params(1, True).items()})
m = m.to(dev).eval()


def spread(exits, t0, span):
    return (exits.max() - exits.mean()) / span, (exits.max() - exits.min()) / span


print("library:", _lib.LIB_PATH)
print("%-8s %3s %9s | %-19s | %-19s | %-19s | units per wave" % ("shape", "rep", "launch ms", "waves  late-mean  late-early",
                                                                 "workgroups", "XCDs"))
with torch.no_grad():
    for name, n_samples in (("fine", 128), ("coarse", 64)):
        torch.manual_seed(0)
        z = torch.sort(torch.rand((rays.shape[0], n_samples), device=dev) * 4 + 2, -1)[0].contiguous()
        rendering._mlp(m, rays, z, False, 0)
        for rep in range(reps):
            stamps.zero_()
            torch.cuda.synchronize()
            rendering._mlp(m, rays, z, False, 0)
            torch.cuda.synchronize()
            s = stamps.cpu().numpy().astype(np.float64)
            s = s[s[:, 1] > 0]                          # waves that ran
            t0 = s[:, 0].min()
            span = s[:, 1].max() - t0                   # 100 MHz ticks
            wave_exit = s[:, 1]
            wg_exit = wave_exit.reshape(-1, 4).max(1)
            xcd = s[:, 2].reshape(-1, 4)[:, 0].astype(int)
            xcd_exit = np.array([wg_exit[xcd == x].max() for x in sorted(set(xcd))])
            xcd_mean = np.array([wg_exit[xcd == x].mean() for x in sorted(set(xcd))])
            cols = ["%.5f  %.5f" % spread(e, t0, span) for e in (wave_exit, wg_exit, xcd_exit)]
            print("%-8s %3d %9.3f | %19s | %19s | %19s | %d..%d" % (name, rep, span / 1e5, cols[0], cols[1], cols[2], s[:, 3].min(), s[:, 3].max()))
            print("         mean workgroup exit per XCD, relative to the latest XCD mean (fraction of the launch):",
                  " ".join("%d:%.5f" % (x, (xcd_mean.max() - v) / span) for x, v in zip(sorted(set(xcd)), xcd_mean)))
