"""More than 64 samples per ray: inputs and acceptance shared by tests/test_per_ray_wide_{cpu,gpu}.py.

The per-ray kernels of csrc/sn_render.hip give one ray to one 64-lane wave; above 64 elements each lane owns
C = ceil(count / 64) CONSECUTIVE ones (lane l: [l C, (l + 1) C)).  Everything here is built to make a wrong
element-to-lane map visible: shapes on both sides of every C the tables below name, weight rows whose only mass sits on the
first or the last element of a lane's chunk, and numpy restatements of the two kernels that carry a cross-lane value
(``emulate_sampler``, ``emulate_composite_backward``) with the map as a parameter, so that the CPU suite can show that the
acceptance functions reject a kernel with the wrong one.
Inputs are well conditioned on purpose (no opaque ray, no sharp surface): the subject is the lane map, not conditioning."""
import numpy as np

from oracle import oracle_np as O
from tests.helpers import sample_pdf_tol, well_conditioned

F, f8 = np.float32, np.float64
WAVE = 64

# (S, NI, deterministic u too).  With fewer than 64 deterministic samples the last one (u == 1) sits on the last cdf knot by
# construction and alone takes more than 3 % of the entries, so (1000, 24) is run with random u only.
SAMPLER_SHAPES = [(67, 64, True), (130, 64, True), (131, 100, True), (200, 128, True), (257, 300, True), (513, 511, True),
                  (1000, 24, False)]
SAMPLER_C = {67: 2, 130: 2, 131: 3, 200: 4, 257: 4, 513: 8, 1000: 16}
FAMILIES = ("cube", "surface", "onehot")
SAMPLER_CASES = [(S, NI, fam, rand_u) for S, NI, det_too in SAMPLER_SHAPES for fam in FAMILIES
                 for rand_u in ((False, True) if det_too else (True,))]
N_SAMPLER_RAYS = 96

COMPOSITE_FWD_S = (65, 257, 513, 960, 1024)
COMPOSITE_BWD_S = (65, 256, 257, 513, 704, 1000, 1024)
BWD_BAR = 2e-5                                     # of max |reference|, the bar of test_composite_backward_vs_oracle


def chunk(count):
    """elements per lane for `count` elements of one ray"""
    return (count + WAVE - 1) // WAVE


def lane_boundaries(count):
    """first and last element of every lane's chunk that is not element 0: C-1, C, 2C-1, 2C, ..., count-1"""
    C = chunk(count)
    b = sorted({k for l in range(WAVE) for k in (l * C, l * C + C - 1) if 0 < k < count} | {count - 1})
    return [k for k in b if k >= C - 1]


# ------------------------------------------------------------------------------------------------ sampler
def sampler_inputs(S, NI, family, rand_u, n=N_SAMPLER_RAYS):
    """(z_coarse (n, S), weights (n, S), u (n, NI) or None): near 2, far 6, stratified depths with perturb = 1; the pdf of the
    sampler is weights[:, 1:-1] (M = S - 2 bins)."""
    r = np.random.RandomState(1000 * S + NI)
    rays = np.zeros((n, 8), F)
    rays[:, 6], rays[:, 7] = 2.0, 6.0
    zc = O.coarse_z_vals(rays, S, False, 1.0, r.uniform(0, 1, (n, S)).astype(F))
    M = S - 2
    if family == "cube":
        w = (r.uniform(0, 1, (n, S)) ** 3).astype(F)
    elif family == "surface":
        centre = r.uniform(0, S, (n, 1))
        w = (np.exp(-0.5 * ((np.arange(S)[None] - centre) / (S / 16.0)) ** 2) + 1e-3).astype(F)
    elif family == "onehot":
        # all of a ray's mass in one pdf bin, which walks over the first and the last bin of every lane's chunk (0, C-1, C,
        # 2C-1, ..., M-1): with a wrong bin-to-lane map nearly every sample of the ray moves, and no exclusion can hide that
        hot = [0] + lane_boundaries(M)
        pick = [hot[i % len(hot)] for i in range(n)] if len(hot) <= n else \
               [hot[i] for i in np.round(np.linspace(0, len(hot) - 1, n)).astype(int)]
        # The hot weight is 4, not 1.  An empty bin has mass eps / (hot + M eps): with hot = 1 that is a hair under the
        # `denom < eps` switch of rendering.py:56, and behind the hot bin (cdf ~ 1, ulp 6e-8) the fp32 cdf differences of such
        # bins fall on either side of eps by their last bit for M < ~600 -- a jump of a bin width that well_conditioned() does
        # not model.  With hot = 4 every empty bin is at eps / 4, 125 ulps clear of the switch.  (A floor under the other bins
        # instead would put them all in the amplified regime, where the comparison measures the reference's fp32 pairwise
        # sum of 1 + many small terms, several ulps off, against the kernel's double sum.)
        w = np.zeros((n, S), F)
        w[np.arange(n), 1 + np.asarray(pick)] = 4.0
    else:
        raise ValueError(family)
    u = r.uniform(0, 1, (n, NI)).astype(F) if rand_u else None
    return zc, w, u


def check_sampler(zc, w, u, NI, z_fine, z_merged, tag=""):
    """Acceptance of one sampler launch (sn_sample_pdf or a restatement of it).  Returns (worst err / tol on the
    well-conditioned entries, their share); raises AssertionError."""
    n, S = zc.shape
    mid = (F(0.5) * (zc[:, :-1] + zc[:, 1:]).astype(F)).astype(F)
    pdf_w = w[:, 1:-1]
    uu = O.linspace01(NI)[None].repeat(n, 0) if u is None else u
    z_fine, z_merged = np.asarray(z_fine), np.asarray(z_merged)
    assert z_fine.shape == (n, NI) and z_merged.shape == (n, S + NI), (tag, z_fine.shape, z_merged.shape)
    assert np.isfinite(z_fine).all(), tag
    assert np.array_equal(z_merged, np.sort(np.concatenate([zc, z_fine], -1), -1)), f"{tag}: merged depths != sort(cat)"
    assert (z_fine >= mid[:, :1] - 1e-6).all() and (z_fine <= mid[:, -1:] + 1e-6).all(), f"{tag}: sample outside its bins"
    ok = well_conditioned(mid, pdf_w, uu)
    share = float(ok.mean())
    assert share >= 0.97, (tag, share)                 # a condition on the inputs, not a measurement
    ref = O.sample_pdf(mid, pdf_w, NI, det=u is None, u=u)
    ratio = np.abs(z_fine.astype(f8) - ref) / sample_pdf_tol(mid, pdf_w, uu)
    worst = float(ratio[ok].max())
    assert worst <= 1.0, f"{tag}: |z_fine - oracle| / tol = {worst:.3g} on a well-conditioned entry"
    return worst, share


def emulate_sampler(zc, w, u, NI, eps=1e-5, strided=False):
    """numpy restatement of sample_pdf_kernel<FROM_Z = true>: total summed in double and rounded once, an fp32 divide, the
    cdf as a double scan (per-lane chunk sums, a scan over the lanes, the chunk again) rounded per element, the binary search,
    the lerp, the merge.  ``strided``: lane l owns bins l, l + 64, ... (k = lane + 64 c) instead of l C .. l C + C - 1 while the
    scan still treats them as consecutive -- the map error the tests must catch.  Returns (z_fine, z_merged)."""
    n, S = zc.shape
    M, L = S - 2, S - 1
    C = chunk(M)
    eps = F(eps)
    wf = (w[:, 1:-1].astype(F) + eps).astype(F)
    tot = wf.astype(f8).sum(-1, keepdims=True).astype(F)
    pdf = np.zeros((n, WAVE * C), f8)
    pdf[:, :M] = (wf / tot).astype(F)
    lane, c = np.meshgrid(np.arange(WAVE), np.arange(C), indexing="ij")
    k = lane + WAVE * c if strided else lane * C + c                     # (64, C): the bin of (lane, c)
    own = pdf[:, k]                                                        # (n, 64, C)
    run = own.sum(-1)
    acc0 = np.cumsum(run, -1) - run                                        # exclusive prefix over the lanes
    incl = acc0[:, :, None] + np.cumsum(own, -1)
    cdf = np.zeros((n, WAVE * C + 1), F)
    cdf[:, 1 + k.reshape(-1)] = incl.reshape(n, -1).astype(F)
    cdf = cdf[:, :L]
    bins = (F(0.5) * (zc[:, :-1] + zc[:, 1:]).astype(F)).astype(F)
    uu = np.ascontiguousarray(O.linspace01(NI)[None].repeat(n, 0) if u is None else u, F)
    lo, hi = np.zeros((n, NI), np.int64), np.full((n, NI), L, np.int64)
    while (lo < hi).any():                                                 # searchsorted(right=True) as the kernel's loop
        act = lo < hi
        m = (lo + hi) >> 1
        le = np.take_along_axis(cdf, np.minimum(m, L - 1), 1) <= uu
        lo = np.where(act & le, m + 1, lo)
        hi = np.where(act & ~le, m, hi)
    below, above = np.maximum(lo - 1, 0), np.minimum(lo, M)
    c0, c1 = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
    b0, b1 = np.take_along_axis(bins, below, 1), np.take_along_axis(bins, above, 1)
    denom = (c1 - c0).astype(F)
    denom = np.where(denom < eps, F(1), denom)
    z_fine = (b0 + (((uu - c0).astype(F) / denom).astype(F) * (b1 - b0).astype(F)).astype(F)).astype(F)
    return z_fine, np.sort(np.concatenate([zc, z_fine], -1), -1, kind="stable")


# ------------------------------------------------------------------------------------------------ compositor
def composite_inputs(S, n_step, sigma_scale, seed=None):
    """The recipe of test_composite_vs_oracle (n_step 7, sigma_scale 3) / test_composite_backward_vs_oracle (9, 2):
    rays, z (n, S) ascending in [2, 6], raw (n, S, 4) = [uniform rgb, normal sigma], noise (n, S), RandomState for more."""
    r = np.random.RandomState(S if seed is None else seed)
    rays = O.lego_rays(30, 30, seed=2)[::n_step]
    n = rays.shape[0]
    z = np.sort(r.uniform(2, 6, (n, S)).astype(F), -1)
    raw = r.uniform(0, 1, (n, S, 4)).astype(F)
    raw[..., 3] = (r.standard_normal((n, S)) * sigma_scale).astype(F)
    noise = r.standard_normal((n, S)).astype(F)
    return rays, z, raw, noise, r


def backward_settings(S):
    """(white_back, noise_std, with g_w) of a sample count: the four combinations of the existing tests, in turn"""
    combos = [(True, 1.0, False), (False, 0.0, True), (True, 0.5, True), (False, 1.0, False)]
    return combos[COMPOSITE_BWD_S.index(S) % 4]


def probe_inputs(S):
    """Position probe of the compositor backward: ray r has g_w = 1 at sample j_r and no other upstream gradient, j_r walking
    over every lane boundary of the shape (C-1, C, 2C-1, ..., S-1).  sigma at the probed sample is made positive so that the
    probed weight exists.  Returns rays, z, raw, g_w, j."""
    j = np.asarray(lane_boundaries(S))
    rays, z, raw, _, _ = composite_inputs(S, 7, 2, seed=S + 5000)
    assert rays.shape[0] >= len(j)
    n = len(j)
    rays, z, raw = rays[:n], z[:n], raw[:n]
    raw[np.arange(n), j, 3] = np.abs(raw[np.arange(n), j, 3]) + F(0.1)
    g_w = np.zeros((n, S), F)
    g_w[np.arange(n), j] = 1.0
    return rays, z, raw, g_w, j


def probe_reference(rays, z, raw, j):
    """float64 dL/d(raw) for L = w_j:  d w_j / d alpha_i = T_j [i == j] - w_j / f_i [i < j], times the sigma factor
    d alpha_i / d sigma_i = delta_i exp(-delta_i sigma_i) [sigma_i > 0]; the rgb columns are zero."""
    n, S = z.shape
    dz = np.concatenate([(z[:, 1:] - z[:, :-1]).astype(F), np.full((n, 1), 1e10, F)], -1)
    d = rays[:, 3:6]
    dnorm = np.sqrt(np.sum((d * d).astype(F), -1, keepdims=True, dtype=F)).astype(F)
    delta = (dz * dnorm).astype(F).astype(f8)
    sig = raw[..., 3]
    e = np.exp(-delta * np.maximum(sig, F(0)).astype(f8))
    f = 1.0 - (1.0 - e) + 1e-10
    T = np.cumprod(np.concatenate([np.ones((n, 1)), f], -1), -1)[:, :-1]
    rows = np.arange(n)
    Tj = T[rows, j]
    wj = (1.0 - e[rows, j]) * Tj
    i = np.arange(S)[None]
    g_alpha = np.where(i == j[:, None], Tj[:, None], 0.0) - np.where(i < j[:, None], wj[:, None] / f, 0.0)
    out = np.zeros((n, S, 4))
    out[..., 3] = g_alpha * delta * e * (sig > 0)
    return out


def emulate_composite_backward(raw, z, rays_d, noise, noise_std, white_back, g_rgb, g_depth, g_w=None, forget_carry_at=None):
    """numpy restatement of composite_bwd_body's g_raw: fp32 elementwise work, the transmittance as a double product scan over
    the lanes rounded per element, the suffix sum of G w as total - inclusive lane scan in double.  ``forget_carry_at`` = b:
    lanes <= b lose what the lanes above b contribute to their suffix -- a scan that drops the carry across the boundary between
    lanes b and b + 1."""
    n, S = z.shape
    C = chunk(S)
    P = WAVE * C
    pad = lambda a, v: np.concatenate([a, np.full((n, P - S) + a.shape[2:], v, a.dtype)], 1)
    valid = np.arange(P)[None] < S
    dz = np.concatenate([(z[:, 1:] - z[:, :-1]).astype(F), np.full((n, 1), 1e10, F)], -1)
    dnorm = np.sqrt(np.sum((rays_d * rays_d).astype(F), -1, keepdims=True, dtype=F)).astype(F)
    d = pad((dz * dnorm).astype(F), F(0))
    rawp, zp = pad(raw.astype(F), F(0)), pad(z.astype(F), F(0))
    sp = rawp[..., 3]
    if noise is not None:
        sp = (sp + pad((noise.astype(F) * F(noise_std)).astype(F), F(0))).astype(F)
    pos = (sp > 0) & valid
    e = np.where(valid, np.exp((-d * np.maximum(sp, F(0))).astype(F)).astype(F), F(1))
    a = (F(1) - e).astype(F)
    f = np.where(valid, ((F(1) - a).astype(F) + F(1e-10)).astype(F), F(1))
    g_rgb, g_depth = g_rgb.astype(F), g_depth.astype(F)
    gwhite = (g_rgb[:, 0] + g_rgb[:, 1] + g_rgb[:, 2]).astype(F) if white_back else np.zeros(n, F)
    G = (g_rgb[:, None, 0] * rawp[..., 0]).astype(F)
    for q in (1, 2):
        G = (G + (g_rgb[:, None, q] * rawp[..., q]).astype(F)).astype(F)
    G = ((G + (g_depth[:, None] * zp).astype(F)).astype(F) - gwhite[:, None]).astype(F)
    if g_w is not None:
        G = (G + pad(g_w.astype(F), F(0))).astype(F)
    G = np.where(valid, G, F(0))
    T = np.cumprod(np.concatenate([np.ones((n, 1)), f.astype(f8)], -1), -1)[:, :-1].astype(F)
    w = (a * T).astype(F)
    Gw = G.astype(f8) * w.astype(f8)
    local = Gw.reshape(n, WAVE, C).sum(-1)
    above = local.sum(-1, keepdims=True) - np.cumsum(local, -1)            # what the higher lanes hold
    if forget_carry_at is not None:
        b = forget_carry_at
        above[:, :b + 1] -= local[:, b + 1:].sum(-1, keepdims=True)
    Gw3 = Gw.reshape(n, WAVE, C)
    within = np.flip(np.cumsum(np.flip(Gw3, -1), -1), -1) - Gw3            # later samples of the same lane
    suffix = (above[:, :, None] + within).reshape(n, P)
    g_alpha = (G.astype(f8) * T.astype(f8) - suffix / f.astype(f8)).astype(F)
    g_sigma = np.where(pos, ((g_alpha * d).astype(F) * e).astype(F), F(0))
    out = np.concatenate([(w[..., None] * g_rgb[:, None, :]).astype(F), g_sigma[..., None]], -1)
    return out[:, :S]


def check_backward(got, ref, tag=""):
    """|got - ref| <= 2e-5 max |ref|; returns err / bar"""
    scale = np.abs(ref).max()
    assert scale > 0, tag
    worst = float(np.abs(np.asarray(got, f8) - ref).max() / (BWD_BAR * scale))
    assert worst <= 1.0, f"{tag}: err / bar = {worst:.3g} (scale {scale:.3g})"
    return worst
