"""Time one optimiser step on the two-NeRF buffer (1 191 688 floats, world size 1): FlatSGD / FlatRAdam / FlatRanger -- one launch over
the flat buffers -- against the same update written as per-parameter torch ops over the 48 tensors on the same device, which is the form
the reference's ``utils/optimizers.py`` (and a stock ``torch.optim.SGD`` without foreach) runs.  The baseline below is this project's
restatement of that loop, not the reference's code; every torch call in it is one kernel launch and is counted as it is issued.

Each step is timed on its own with a host clock around step + device synchronise; the two forms alternate step by step, so both see the
same machine.  Reported: the median of ``--steps`` (default 200) steps after ``--warmup`` (default 20, which also takes RAdam / Ranger
past their five degenerate steps), launches per step, and the bytes the flat kernel moves per step.

usage: python tools/optim_time.py [--steps 200] [--warmup 20] [--out FILE.json]        (needs the GPU; there is no CPU form)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LR, WD, EPS, MOMENTUM, ALPHA, K = 5e-4, 1e-3, 1e-8, 0.9, 0.5, 6
BETAS = {"radam": (0.9, 0.999), "ranger": (0.95, 0.999)}
# fp32 arrays the flat kernel reads + writes per element: p (r, w), g (r), state (r, w each); Ranger's slow buffer only on a lookahead step
ARRAYS = {"sgd": 5, "radam": 7, "ranger": 7, "ranger_sync": 9}


class PerTensor:
    """the per-parameter form: a Python loop over the tensors, one torch op (= one launch) per line of the update rule"""

    def __init__(self, kind, params):
        self.kind, self.params, self.step_count, self.launches = kind, params, 0, 0
        self.state = [{k: torch.zeros_like(p) for k in (("buf",) if kind == "sgd" else ("m", "v"))} for p in params]
        if kind == "ranger":
            for st, p in zip(self.state, params):
                st["slow"] = p.detach().clone()

    @torch.no_grad()
    def step(self):
        from sinnerf_amd.optim import radam_step_scalars
        self.step_count += 1
        n = 0
        if self.kind != "sgd":
            b1, b2 = BETAS[self.kind]
            _, _, rect, coeff, decay = radam_step_scalars(self.step_count, LR, (b1, b2), WD, strict=self.kind == "ranger")
        for p, st in zip(self.params, self.state):
            g = p.grad
            if self.kind == "sgd":
                g = g.add(p, alpha=WD); n += 1
                st["buf"].mul_(MOMENTUM); n += 1
                st["buf"].add_(g); n += 1
                p.add_(st["buf"], alpha=-LR); n += 1
                continue
            st["v"].mul_(b2); n += 1
            st["v"].addcmul_(g, g, value=1 - b2); n += 1
            st["m"].mul_(b1); n += 1
            st["m"].add_(g, alpha=1 - b1); n += 1
            p.add_(p, alpha=-decay); n += 1
            if rect:
                denom = st["v"].sqrt(); n += 1
                denom.add_(EPS); n += 1
                p.addcdiv_(st["m"], denom, value=-coeff); n += 1
            else:
                p.add_(st["m"], alpha=-coeff); n += 1
            if self.kind == "ranger" and self.step_count % K == 0:
                d = p - st["slow"]; n += 1
                st["slow"].add_(d, alpha=ALPHA); n += 1
                p.copy_(st["slow"]); n += 1
        self.launches = n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_time.py needs the GPU: a CPU run measures nothing")
    from sinnerf_amd import NeRF
    from sinnerf_amd.optim import FlatRAdam, FlatRanger, FlatSGD
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "kinds": {}}
    for kind in ("sgd", "radam", "ranger"):
        torch.manual_seed(0)
        fa = [NeRF(use_new_activation=True).to(dev), NeRF(use_new_activation=True).to(dev)]
        fb = [NeRF(use_new_activation=True).to(dev), NeRF(use_new_activation=True).to(dev)]
        if kind == "sgd":
            flat = FlatSGD(fa, lr=LR, momentum=MOMENTUM, weight_decay=WD)
        elif kind == "radam":
            flat = FlatRAdam(fa, lr=LR, eps=EPS, weight_decay=WD)
        else:
            flat = FlatRanger(fa, lr=LR, eps=EPS, weight_decay=WD)
        n = flat.flat.numel()
        flat.grads.flat.normal_(0.0, 0.01)
        params = [p for m in fb for p in m.parameters()]
        for p in params:
            p.grad = torch.randn_like(p) * 0.01
        base = PerTensor(kind, params)
        times = {"flat": [], "per_tensor": []}
        sync_steps = []
        for it in range(a.warmup + a.steps):
            for name, opt in (("flat", flat), ("per_tensor", base)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                opt.step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if it >= a.warmup:
                    times[name].append(dt)
            if it >= a.warmup:
                sync_steps.append(kind == "ranger" and flat.step_count % K == 0)
        r = {"n": n, "tensors": len(params), "flat_launches": 1, "per_tensor_launches_plain_step": None,
             "flat_bytes": ARRAYS[kind] * 4 * n}
        # launches of a step without lookahead: recount on a step known to be plain
        while kind == "ranger" and (base.step_count + 1) % K == 0:
            base.step()
        base.step()
        r["per_tensor_launches_plain_step"] = base.launches
        for name, ts in times.items():
            plain = [t for t, s in zip(ts, sync_steps) if not s]
            r[name + "_median_us"] = 1e6 * statistics.median(plain)
            r[name + "_p10_us"], r[name + "_p90_us"] = (1e6 * q for q in (statistics.quantiles(plain, n=10)[0], statistics.quantiles(plain, n=10)[-1]))
            if kind == "ranger":
                r[name + "_lookahead_median_us"] = 1e6 * statistics.median([t for t, s in zip(ts, sync_steps) if s])
        if kind == "ranger":
            r["flat_bytes_lookahead"] = ARRAYS["ranger_sync"] * 4 * n
            r["per_tensor_launches_lookahead_step"] = r["per_tensor_launches_plain_step"] + 3 * len(params)
        r["flat_gbps_at_median"] = r["flat_bytes"] / (r["flat_median_us"] * 1e-6) / 1e9
        result["kinds"][kind] = r
        print("%-6s flat: %7.1f us (p10 %.1f, p90 %.1f; 1 launch, %.2f MB moved, %.0f GB/s incl. launch + sync)   per-tensor torch ops: "
              "%8.1f us (%d launches over %d tensors)   ratio %.1fx" % (
                  kind, r["flat_median_us"], r["flat_p10_us"], r["flat_p90_us"], r["flat_bytes"] / 1e6, r["flat_gbps_at_median"],
                  r["per_tensor_median_us"], r["per_tensor_launches_plain_step"], len(params), r["per_tensor_median_us"] / r["flat_median_us"]))
        if kind == "ranger":
            print("       lookahead steps: flat %.1f us, per-tensor %.1f us (%d launches)" % (
                r["flat_lookahead_median_us"], r["per_tensor_lookahead_median_us"], r["per_tensor_launches_lookahead_step"]))
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
