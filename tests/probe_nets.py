"""Probe networks for the range tests of the fused MLP kernels (tests/test_probe_nets_cpu.py, tests/test_mlp_range_gpu.py): parameter sets
in the reference's ``state_dict`` shapes (models/nerf.py:66-103) with which the pre-activations of the two heads are EXACTLY known
functions of the input in every arithmetic the kernels implement, the fp64 values the heads must then produce, and the per-element bars.

Head probe.  ``O.init_params(seed, True)`` (a live trunk, so sigma is an ordinary output) with xyz_encoding_final and dir_encoding zeroed
except: dir_encoding channel j_k reads ONE identity column of the direction embedding (input column 256 + k) with a power-of-two weight
a_k and a bias b_k; rgb row o reads ONE channel, W[o, j_o] = s_o, bias b3_o.  With directions that are multiples of 1/64 (exact in bf16)

    y2[:, j_k] = a_k d_k + b_k   (every other channel: 0),      y3[:, o] = s_o act2(y2[:, j_o]) + b3_o

-- y2 exactly (one product by a power of two, one exact sum), y3 up to the one rounding of its fp32 sum.  The inputs the other tests feed
the heads keep y2 inside [-0.5, 0.5] and y3 inside [-0.2, 0.4]; here y2 spans [-32, 32] and y3 [-30, 24].

Embedding probe (inference kernels: they do not store the embedding).  Layer 1 takes embedding column c into two channels with weights
+1 / -1, layers 2..8 are the identity on those two channels, sigma = h[0] - h[1], every bias 0: sigma = relu(E_c) - relu(-E_c) = E_c,
rounded once to the operand format in the 16-bit arithmetics."""
import numpy as np

from oracle import oracle_np as O

F = np.float32

# ---- head probe ------------------------------------------------------------------------------------------------------------------
N_RAYS, N_SAMPLES = 321, 5                    # 1605 points: ragged for 128- and 256-point tiles
# name -> (init seed, dir_encoding channels j_k (both lane halves: j < 64 and j >= 64), (a_k, b_k), (s_o, b3_o))
HEAD_SETS = {
    "wide": (0, (5, 70, 127), ((16.0, 0.0), (1.0, 1.0), (-4.0, 2.0)), ((1.0, -8.0), (2.0, -3.0), (-1.0, 4.0))),      # y3 in [-8, 24]
    "low": (3, (64, 3, 100), ((16.0, 0.0), (1.0, 1.0), (-4.0, 2.0)), ((-1.0, 1.0), (4.0, -12.0), (-2.0, 8.0))),      # y3 down to -30
}
E_REF = 1.04e-7                               # the oracle's own fp32 rgb against fp64 on the "wide" set (tests/test_probe_nets_cpu.py)


def head_params(name):
    seed, chans, ab, sb3 = HEAD_SETS[name]
    p = O.init_params(seed, True)
    for k in ("xyz_encoding_final.weight", "xyz_encoding_final.bias", "dir_encoding.0.weight", "dir_encoding.0.bias",
              "rgb.0.weight", "rgb.0.bias"):
        p[k] = np.zeros_like(p[k])
    for k, (j, (a, b), (s, b3)) in enumerate(zip(chans, ab, sb3)):
        p["dir_encoding.0.weight"][j, 256 + k] = a
        p["dir_encoding.0.bias"][j] = b
        p["rgb.0.weight"][k, j] = s
        p["rgb.0.bias"][k] = b3
    return p


def head_rays():
    """(rays (321, 8), z (321, 5)): direction components = the 257 multiples of 1/64 in [-2, 2] in three different orders (not unit
    vectors: no kernel normalises them), origins and depths that keep the points where the other tests have them."""
    r = np.arange(N_RAYS)
    d = np.stack([((r * m + off) % 257 - 128) / 64.0 for m, off in ((1, 0), (100, 31), (37, 200))], 1)
    rs = np.random.RandomState(12)
    rays = np.concatenate([rs.uniform(-1, 1, (N_RAYS, 3)), d, np.full((N_RAYS, 1), 0.5), np.full((N_RAYS, 1), 1.5)], 1).astype(F)
    z = np.sort(rs.uniform(0.5, 1.5, (N_RAYS, N_SAMPLES)), -1).astype(F)
    return rays, z


def head_inputs():
    """rays, z and the pre-embedded rows (1605, 90) of the same points (the input of the *_embedded entries)"""
    rays, z = head_rays()
    x = np.concatenate([O.embedding(O._points(rays, z).reshape(-1, 3), 10), np.repeat(O.embedding(rays[:, 3:6], 4), N_SAMPLES, 0)], 1)
    return rays, z, np.ascontiguousarray(x, F)


def softplus64(x):
    """ShiftedSoftplus's softplus(x) = log1p(exp(-|x|)) + max(x, 0) in fp64"""
    x = np.asarray(x, np.float64)
    return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0)


_SCALE = np.float64(F(1.0 + 2.0 * 1e-3))      # WidenedSigmoid's 1 + 2 eps as the fp32 constant every implementation multiplies with


def head_reference(name, classic=False, d_cols=None):
    """fp64 values of everything the heads compute for the probe points, as a dict of (1605, 3) arrays indexed by rgb row o (its channel
    is chans[o]):  y2, h2 = act2(y2), y3, rgb, D2 = act2'(y2), D3 = act3'(y3), s; plus h2_rest = act2(0), the value of every other channel.
    d_cols: (1605, 3) values of the three identity columns (default: the ray directions of head_rays())."""
    _, chans, ab, sb3 = HEAD_SETS[name]
    if d_cols is None:
        d_cols = np.repeat(head_rays()[0][:, 3:6], N_SAMPLES, 0)
    d = np.asarray(d_cols, np.float64)
    a, b = np.array(ab, np.float64).T
    s, b3 = np.array(sb3, np.float64).T
    with np.errstate(over="ignore"):                # exp of a large argument: inf, and the quotient is the right 0
        y2 = a * d + b
        if classic:                                # nerf.py:91-100: ReLU / Sigmoid
            h2, D2, rest = np.maximum(y2, 0.0), (y2 > 0).astype(np.float64), 0.0
        else:
            h2, D2, rest = softplus64(y2 - 1.0), 1.0 / (1.0 + np.exp(-(y2 - 1.0))), float(softplus64(-1.0))
        y3 = s * h2 + b3
        if classic:
            rgb = 1.0 / (1.0 + np.exp(-y3))
            D3 = rgb * (1.0 - rgb)
        else:
            t = np.tanh(0.5 * y3)
            rgb = 0.5 * (1.0 + _SCALE * t)
            D3 = 0.25 * _SCALE * (1.0 - t * t)
    return dict(y2=y2, h2=h2, y3=y3, rgb=rgb, D2=D2, D3=D3, s=np.broadcast_to(s, y2.shape), h2_rest=rest, chans=chans)


_SIGNIFICAND_BITS = {"bf16": 8, "fp16": 11, "bf16x3": 16}      # bf16x3: a (hi, lo) pair of bf16 values


def operand_half_ulp(ref, arith):
    """Half an ulp of the operand format at |ref|, per element: what ONE round-to-nearest of ref to that format may move it by --
    2^(e - p) with 2^e <= |ref| < 2^(e + 1) and p significand bits (relative to |ref| between 2^-(p + 1) at the top of a binade -- 2^-9 for
    bf16, 2^-12 for fp16, 2^-17 for the bf16 pair -- and 2^-p at its bottom); fp16 is subnormal below 2^-14 (half an ulp: 2^-25)."""
    ref = np.abs(np.asarray(ref, np.float64))
    if arith == "fp32":
        return np.zeros_like(ref)
    e = np.frexp(ref)[1] - 1
    half = np.where(ref > 0, np.ldexp(1.0, e - _SIGNIFICAND_BITS[arith]), 0.0)
    return np.maximum(half, 2.0 ** -25) if arith == "fp16" else half


def softplus_bar(ref, bf16_state=False):
    """3.6e-6 |ref| + 1.2e-7: twice the documented bounds of the kernels' two softplus forms (relative 1.8e-6, sn_mlp_pipe.h; absolute
    2^-24, sn_mlp_bf16.h); a value stored as bf16 adds half a bf16 ulp"""
    ref = np.abs(np.asarray(ref, np.float64))
    return 3.6e-6 * ref + 1.2e-7 + (operand_half_ulp(ref, "bf16") if bf16_state else 0.0)


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64)).astype(F)
    return (np.nextafter(x, F(np.inf)) - x).astype(np.float64)


def rgb_bar(ref, classic=False):
    """4 E_ref + (the softplus bar through s + one ulp of y3) times the activation's fp64 slope at y3"""
    h2_bar = 0.0 if classic else softplus_bar(ref["h2"])
    return 4 * E_REF + (np.abs(ref["s"]) * h2_bar + ulp32(ref["y3"])) * ref["D3"]


def g_y3_bar(ref, g_rgb, classic=False, bf16_state=False):
    """|g| (bar(rgb) + 2^-22): the derivative is rebuilt from the stored colour (its slope in the colour is at most 1)"""
    val = np.abs(g_rgb * ref["D3"])
    return np.abs(g_rgb) * (rgb_bar(ref, classic) + 2.0 ** -22) + (operand_half_ulp(val, "bf16") if bf16_state else 0.0)


def g_y2_bar(ref, g_y3, classic=False, bf16_state=False):
    """|g_h2| (bar(h2) + 2^-22) + 2^-22 |ref| with g_h2 = s g_y3 (an exact product: s is a power of two) from the g_y3 the chain itself
    wrote to g_out -- the two roundings of 1 - exp(-h2) on the STORED h2; a value stored as bf16 adds half a bf16 ulp"""
    g_h2 = ref["s"] * g_y3
    val = np.abs(g_h2 * ref["D2"])
    h2_bar = 0.0 if classic else softplus_bar(ref["h2"], bf16_state)
    return np.abs(g_h2) * (h2_bar + 2.0 ** -22) + 2.0 ** -22 * val + (operand_half_ulp(val, "bf16") if bf16_state else 0.0)


def regime_counts(y2):
    """how many values of y2 - 1 fall below -17 (1 + e rounds to 1), in (-17, -1], (-1, 1], (1, 17], above 17"""
    x = np.asarray(y2, np.float64).ravel() - 1.0
    edges = (-np.inf, -17.0, -1.0, 1.0, 17.0, np.inf)
    return [int(((x > lo) & (x <= hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])]


# ---- embedding probe ---------------------------------------------------------------------------------------------------------------
def embedding_params(c):
    """sigma = E_c, column c of Embedding(3, 10) (c < 63)"""
    p = {k: np.zeros(shp, F) for k, shp in O.param_shapes().items()}
    p["xyz_encoding_1.0.weight"][0, c], p["xyz_encoding_1.0.weight"][1, c] = 1.0, -1.0
    for i in range(2, 9):
        off = 63 if i == 5 else 0              # nerf.py:133: the skip layer reads cat([input_xyz, h])
        p[f"xyz_encoding_{i}.0.weight"][0, off], p[f"xyz_encoding_{i}.0.weight"][1, off + 1] = 1.0, 1.0
    p["sigma.weight"][0, 0], p["sigma.weight"][0, 1] = 1.0, -1.0
    return p


def dir_column_params(name, c):
    """the head probe `name` with its three dir_encoding channels reading column c of Embedding(3, 4) (c < 27): y2 = a E_c + b"""
    p = head_params(name)
    _, chans, ab, _ = HEAD_SETS[name]
    for k, (j, (a, _)) in enumerate(zip(chans, ab)):
        p["dir_encoding.0.weight"][j, 256 + k] = 0.0
        p["dir_encoding.0.weight"][j, 256 + c] = a
    return p


def probe_values(n, seed):
    """(n, 3) fp32 coordinates at the magnitudes a real scene has: +-0, exact powers of two, the fp32 neighbours of k pi / 2^b for the
    ten bands (the zeros and extrema of sin / cos(2^b x), where a range reduction is at its worst), and the rest log-uniform in sign and
    magnitude over 1e-3 .. 1e3"""
    pool = [0.0, -0.0] + [sg * 2.0 ** e for e in range(-10, 10) for sg in (1, -1)]
    for b in range(10):
        for k in (1, 2, 3, 5, 8, 13, 100, 1001, 30000, 162000):
            v = F(k * np.pi / 2.0 ** b)
            if v <= 1e3:
                pool += [sg * float(w) for w in (np.nextafter(v, F(0)), v, np.nextafter(v, F(np.inf))) for sg in (1, -1)]
    pool = np.array(pool, F)
    assert len(pool) < n
    rs = np.random.RandomState(seed)
    rest = (rs.choice([-1.0, 1.0], (n - len(pool), 3)) * 10.0 ** rs.uniform(-3, 3, (n - len(pool), 3))).astype(F)
    return np.concatenate([np.stack([np.roll(pool, 17 * i) for i in range(3)], 1), rest], 0)


def embedding64(x, n_freqs):
    """Embedding(3, n_freqs) of the exact fp32 arguments in fp64 (2^b x is exact)"""
    x = np.asarray(x, F).astype(np.float64)
    out = [x]
    for b in range(n_freqs):
        out += [np.sin(2.0 ** b * x), np.cos(2.0 ** b * x)]
    return np.concatenate(out, -1)


EMB_BAR_EXACT = 4e-7      # fp32 / bf16x3 kernels (to_revolutions / sincos_rev of sn_device.h), |x| <= 1e3; an fp32 emulation gives 1.9e-7
EMB_BAR_DOUBLING = 2e-5   # bf16 / fp16 kernels (higher bands by angle doubling): the bar of tests/test_grads_gpu.py
