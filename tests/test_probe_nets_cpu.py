"""CPU: the claims tests/probe_nets.py makes about its parameter sets, checked through the numpy oracle in all four arithmetics and both
head variants -- the pre-activations of the heads are the stated functions of the input bit for bit, the probe reaches every regime of
the softplus, and the oracle's own fp32 colours sit within 2e-7 of the fp64 ones (E_ref, the yardstick of the rgb bars of
tests/test_mlp_range_gpu.py)."""
import contextlib

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import probe_nets as PN

ARITHMETICS = {"fp32": contextlib.nullcontext, "bf16": O.bf16_operands, "fp16": O.fp16_operands, "bf16x3": O.bf16x3_operands}


@pytest.fixture(scope="module")
def inputs():
    return PN.head_inputs()


@pytest.mark.parametrize("name", sorted(PN.HEAD_SETS))
@pytest.mark.parametrize("classic", [False, True])
@pytest.mark.parametrize("arith", sorted(ARITHMETICS))
def test_head_pre_activations_are_exact(inputs, name, classic, arith):
    rays, z, x = inputs
    ref = PN.head_reference(name, classic)
    cache = {}
    with ARITHMETICS[arith](), (O.classic_heads() if classic else contextlib.nullcontext()):
        out = O.nerf_forward(PN.head_params(name), x, cache=cache)
    chans = list(ref["chans"])
    assert cache["y2"].dtype == np.float32 and np.array_equal(cache["y2"][:, chans].astype(np.float64), ref["y2"])
    rest = np.delete(cache["y2"], chans, 1)
    assert rest.shape == (x.shape[0], 125) and not rest.any() and not cache["final"].any()
    # y3 is the fp64 value up to the rounding of h2 and of its own sum; the colours follow
    assert np.abs(cache["y3"] - ref["y3"]).max() <= np.abs(ref["s"]).max() * 4e-6 * np.abs(ref["h2"]).max() + 4e-6
    assert np.abs(out[:, :3] - ref["rgb"]).max() <= 2e-7
    assert np.isfinite(out).all() and np.abs(out[:, 3]).max() > 0.1          # the trunk is live: sigma is an ordinary output


def test_head_probe_reaches_every_regime():
    wide, low = PN.head_reference("wide"), PN.head_reference("low")
    for ref in (wide, low):
        counts = PN.regime_counts(ref["y2"])
        print("values of y2 - 1 below -17, in (-17, -1], (-1, 1], (1, 17], above 17:", counts)
        assert sum(counts) == 3 * PN.N_RAYS * PN.N_SAMPLES == 4815
        assert min(counts) >= 0.05 * sum(counts), counts
        assert ref["y2"].min() == -32.0 and ref["y2"].max() == 32.0
    assert wide["y3"].min() <= -8.0 + 1e-6 and wide["y3"].max() >= 22.9, (wide["y3"].min(), wide["y3"].max())
    assert low["y3"].min() <= -30.0 + 1e-6, low["y3"].min()
    # colours at both ends of the activation (a real scene has them at 0 and 1), new heads and classic ones
    for name in PN.HEAD_SETS:
        for classic in (False, True):
            rgb = PN.head_reference(name, classic)["rgb"]
            assert rgb.min() < 1e-3 and (name == "low" or rgb.max() > 1 - 1e-9), (name, classic, rgb.min(), rgb.max())
    # every direction component is a multiple of 1/64 inside [-2.5, 2.5]: exact in bf16 (8 significand bits)
    d = PN.head_rays()[0][:, 3:6]
    assert np.array_equal(d * 64, np.round(d * 64)) and np.abs(d).max() <= 2.5 and np.array_equal(O.bf16_round(d), d)


def test_oracle_fp32_colours_against_fp64(inputs):
    """E_ref: what the oracle's own fp32 heads (the reference's formulas in numpy fp32) lose against fp64"""
    rays, z, x = inputs
    worst = {}
    for name in sorted(PN.HEAD_SETS):
        for classic in (False, True):
            with (O.classic_heads() if classic else contextlib.nullcontext()):
                out = O.nerf_forward(PN.head_params(name), x)
            worst[name, classic] = float(np.abs(out[:, :3] - PN.head_reference(name, classic)["rgb"]).max())
    print("oracle fp32 rgb against fp64:", {k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) <= 2e-7, worst
    assert PN.E_REF <= 2e-7                    # the constant of the GPU bars: worst["wide", False] as first measured (1.04e-7), inside this bound


@pytest.mark.parametrize("arith", sorted(ARITHMETICS))
def test_embedding_probe_returns_the_column(arith):
    pts = PN.probe_values(600, 5)
    e = O.embedding(pts, 10)
    for c in (0, 2, 3, 7, 33, 57, 62):
        with ARITHMETICS[arith]():
            sig = O.nerf_forward(PN.embedding_params(c), e, sigma_only=True)[:, 0]
        if arith == "fp32":
            assert np.array_equal(sig, e[:, c]), c
        else:
            err, bar = np.abs(sig.astype(np.float64) - e[:, c]), PN.operand_half_ulp(e[:, c], arith)
            assert (err <= bar).all(), c
            assert (err > 0.45 * bar).any(), c          # the bar is the format's own half-ulp, reached by round-to-nearest


def test_dir_column_probe_is_exact_in_fp32(inputs):
    """y2 = a E_c + b through any column of Embedding(3, 4): one product by a power of two and one rounded sum"""
    rays, z, x = inputs
    for c in (0, 4, 26):
        cache = {}
        O.nerf_forward(PN.dir_column_params("wide", c), x, cache=cache)
        _, chans, ab, _ = PN.HEAD_SETS["wide"]
        for j, (a, b) in zip(chans, ab):
            assert np.array_equal(cache["y2"][:, j], (np.float32(a) * x[:, 63 + c] + np.float32(b)).astype(np.float32))


def test_probe_values_hold_the_special_points():
    p = PN.probe_values(1605, 1)
    assert p.shape == (1605, 3) and p.dtype == np.float32 and np.isfinite(p).all()
    a = np.abs(p[p != 0])
    assert a.min() >= 2.0 ** -10 * 0.999 and a.max() <= 1e3 and (p == 0).sum() >= 6 and np.signbit(p[p == 0]).any()
    for b in range(10):                        # a zero of sin(2^b x) next to a representable point, in every band
        assert (np.abs(np.sin(2.0 ** b * p[:, 0].astype(np.float64))) < 2.0 ** b * 1e-6).sum() >= 3, b
    m = np.abs(p[400:])
    assert (m < 1e-2).mean() > 0.1 and (m > 1e2).mean() > 0.1
