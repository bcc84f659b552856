"""GPU: the heads and the embedding of the fused MLP kernels against fp64 BEYOND the ranges every other test feeds them (those keep the
dir_encoding pre-activation y2 inside [-0.5, 0.5], the rgb pre-activation y3 inside [-0.2, 0.4] and |x| below 3.7) -- the linear branch
of ShiftedSoftplus in its three implementations, the saturation of WidenedSigmoid / Sigmoid, the derivative forms the backward chain
rebuilds from stored outputs (1 - exp(-h2), .2505 (1 - t^2), y (1 - y)), and to_revolutions / sincos_rev plus the angle-doubling path at
|x| up to 1e3.  The probe networks of tests/probe_nets.py make y2 and y3 exactly known functions of the input (y2 in [-32, 32], y3 in
[-30, 24]) and turn sigma into one embedding column; the C ABI is called directly with the (dtype, flags, sigma_only) rows of the
routing table of tests/test_api_routing_cpu.py, and the last test asserts that all 32 exported launchers (20 forward, 12 chain) ran.

Bars (per element, fp64, tests/probe_nets.py): softplus values 3.6e-6 |ref| + 1.2e-7 (twice the kernels' documented bounds; a bf16-stored
value adds half a bf16 ulp); rgb 4 E_ref + the softplus bar through s and the activation's slope + one ulp of y3 times that slope;
g_y3 |g| (bar(rgb) + 2^-22); g_y2 |g_h2| (bar(h2) + 2^-22) + 2^-22 |ref|; exact-path embedding 4e-7, doubling path 2e-5, probe outputs
plus the operand half-ulp (per element: tests/probe_nets.py operand_half_ulp).  Every test prints its worst err / bar.

Measured on one MI355X (worst err / bar; DESIGN.md §2 item 4 has the table): softplus in slot 9 0.04 (shifted_softplus_fast), 0.50
(ssp4_rgb), bf16 state 0.999 (the store's own rounding); rgb 0.237 (9.9e-8) with the ShiftedSoftplus / WidenedSigmoid heads, 0.175 classic;
g_y3 0.16 (2.0e-7); g_y2 0.10 fp32, 0.20 bf16 operands and bf16x3, classic heads exact; exact-path embedding 1.5e-7 of 4e-7, doubling path
5.4e-6 of 2e-5; identity columns bit-equal; embedding probe 0.38 fp32, 0.49 bf16x3, 0.94 fp16, 0.99 bf16 (operand rounding); dir columns
through the head probe up to 0.99.  Nothing left its bar."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import oracle_np as O                                                                     # noqa: E402
from tests import probe_nets as PN                                                                    # noqa: E402
from tests.helpers import x3_state_to_fp32                                                            # noqa: E402
from tests.test_api_routing_cpu import (BF16, C, CHAIN, EMB, F16, F32, FORWARD, FORWARD_EMBEDDED, ROUTES, STATE, TRAIN,      # noqa: E402
                                        TRAIN_EMBEDDED, X3)
from tests.test_parity_gpu import dev                                                                 # noqa: E402
from tests.test_training_kernels_system_gpu import _emb_dir_pos, _emb_xyz_pos                         # noqa: E402

ARITH = {F32: "fp32", BF16: "bf16", STATE: "bf16", X3: "bf16x3", F16: "fp16"}
EXERCISED = set()             # launcher symbols (without "_launch") the tests of this module handed work to
WORST = {}                    # what -> worst err / bar seen


def _cases(entry):
    """the rows of the routing table an entry accepts, once each (flags / sigma_only are arguments of the inference entries only)"""
    seen = []
    for (dtype, flags, sigma_only, n), want in ROUTES[entry]:
        key = (dtype, flags, sigma_only) if entry in (FORWARD, FORWARD_EMBEDDED) else (dtype, 0, 0)
        if want is not None and n == 1000 and key not in seen:
            seen.append(key)
    return seen


_ENTRY_NAMES = ("forward", "forward_embedded", "train", "train_embedded", "chain")
INFERENCE_CASES = [pytest.param(e, *k, id="%s-dtype%#x-flags%d-sigma%d" % ((_ENTRY_NAMES[e],) + k)) for e in (FORWARD, FORWARD_EMBEDDED) for k in _cases(e)]
TRAINING_CASES = [pytest.param(e, k[0], id="%s-dtype%#x" % (_ENTRY_NAMES[e], k[0])) for e in (TRAIN, TRAIN_EMBEDDED) for k in _cases(e)]
RAY_FORWARD_CASES = [pytest.param(*k, id="dtype%#x-flags%d-sigma%d" % k) for k in _cases(FORWARD)]


def _note(what, err, bar):
    """print and keep the worst err / bar (elements whose bar is 0 must be exact), then assert it"""
    err, bar = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bar, np.float64))
    assert np.isfinite(err).all(), what
    ratio = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    print("%-60s worst err / bar %.3f (max err %.3e)" % (what, ratio, err.max() if err.size else 0.0))
    assert (err <= bar).all(), (what, ratio, float(err.max()))


_MODELS = {}


def _model(arith, params=None):
    import sinnerf_amd
    if arith not in _MODELS:
        _MODELS[arith] = sinnerf_amd.NeRF(use_new_activation=True, compute_dtype=arith).to(dev()).eval()
    if params is not None:
        _MODELS[arith].load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})      # in place: the blobs are re-packed
    return _MODELS[arith]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _launcher(entry, dtype, flags, sigma_only, n):
    from sinnerf_amd import _lib
    name = _lib.lib.sn_mlp_route(entry, dtype, flags, sigma_only, n)
    assert name is not None, (entry, hex(dtype))
    return name.decode()


def _forward(entry, dtype, flags, sigma_only, rays, z, x, params=None):
    """sn_mlp_forward / sn_mlp_forward_embedded; returns (P, 4) or (P,) as numpy"""
    from sinnerf_amd import _lib
    m = _model(ARITH[dtype & 0xff], params)
    P = rays.shape[0] * z.shape[1]
    out = torch.full((P,) if sigma_only else (P, 4), float("nan"), device=dev())
    if entry == FORWARD:
        _lib.check(_lib.lib.sn_mlp_forward(_lib.ptr(m.packed()), dtype, _lib.ptr(rays), _lib.ptr(z), rays.shape[0], z.shape[1], sigma_only,
                                           flags, _lib.ptr(out), _lib.stream_ptr()), "sn_mlp_forward")
    else:
        _lib.check(_lib.lib.sn_mlp_forward_embedded(_lib.ptr(m.packed()), dtype, _lib.ptr(x), P, x.shape[1], sigma_only, flags, _lib.ptr(out),
                                                    _lib.stream_ptr()), "sn_mlp_forward_embedded")
    torch.cuda.synchronize()
    EXERCISED.add(_launcher(entry, dtype, flags, sigma_only, P))
    return out.cpu().numpy()


def _train(entry, dtype, rays, z, x, params=None):
    """sn_mlp_forward_train / _embedded with NaN-filled outputs and state; returns the device tensors (out, acts, emb)"""
    from sinnerf_amd import _lib
    m = _model(ARITH[dtype & 0xff], params)
    n, s = z.shape
    P = n * s
    rows = -(-P // 256) * 256
    state16 = (dtype & 0xff) == STATE
    out = torch.full((P, 4), float("nan"), device=dev())
    acts = torch.full((10, rows, 256), float("nan"), dtype=torch.bfloat16 if state16 else torch.float32, device=dev())
    emb = torch.full((rows, 128), float("nan"), dtype=torch.bfloat16 if dtype & EMB else torch.float32, device=dev())
    if entry == TRAIN:
        _lib.check(_lib.lib.sn_mlp_forward_train(_lib.ptr(m.packed()), dtype, _lib.ptr(rays), _lib.ptr(z), n, s, _lib.ptr(out), _lib.ptr(acts),
                                                 _lib.ptr(emb), rows, _lib.stream_ptr()), "sn_mlp_forward_train")
    else:
        _lib.check(_lib.lib.sn_mlp_forward_train_embedded(_lib.ptr(m.packed()), dtype, _lib.ptr(x), P, x.shape[1], _lib.ptr(out), _lib.ptr(acts),
                                                          rows, _lib.stream_ptr()), "sn_mlp_forward_train_embedded")
    torch.cuda.synchronize()
    EXERCISED.add(_launcher(entry, dtype, 0, 0, P))
    return out, acts, emb


def _state_np(t, dtype):
    """a (10, rows, 256) state array as the fp32 values it holds"""
    if (dtype & 0xff) == STATE:
        return t.float().cpu().numpy()
    a = t.cpu().numpy()
    return x3_state_to_fp32(a) if (dtype & 0xff) == X3 else a


@pytest.fixture(scope="module")
def probe():
    rays, z, x = PN.head_inputs()
    return dict(rays=_t(rays), z=_t(z), x=_t(x), x_np=x, sigma={})


def _check_sigma(probe, got, name, arith, train, what):
    """sigma of the live trunk against the oracle at the bar of the launcher's own parity test"""
    for a in (arith, "fp32"):
        if (name, a) not in probe["sigma"]:
            ctx = {"fp32": None, "bf16": O.bf16_operands, "fp16": O.fp16_operands, "bf16x3": O.bf16x3_operands}[a]
            if ctx is None:
                probe["sigma"][name, a] = O.nerf_forward(PN.head_params(name), probe["x_np"][:, :63], sigma_only=True)[:, 0].astype(np.float64)
            else:
                with ctx():
                    probe["sigma"][name, a] = O.nerf_forward(PN.head_params(name), probe["x_np"][:, :63], sigma_only=True)[:, 0].astype(np.float64)
    ref, ref32 = probe["sigma"][name, arith], probe["sigma"][name, "fp32"]
    if arith in ("fp32", "bf16x3"):           # tests/test_parity_gpu.py test_mlp_forward_vs_oracle, tests/test_bf16x3_gpu.py: against the fp32 oracle
        _note(what + " sigma", np.abs(got - ref32), 2e-4 * (np.abs(ref32) + 1e-3))
    else:                                      # against the oracle with the same operand roundings: test_parity_gpu / test_fp16_gpu / the training tests
        rel = 2.5e-4 if arith == "fp16" else 6e-3 if train else 2e-3
        _note(what + " sigma", np.abs(got - ref), rel * np.abs(ref32).max())


def _check_rgb(got, name, classic, what):
    ref = PN.head_reference(name, classic)
    _note(what + " rgb", np.abs(got - ref["rgb"]), PN.rgb_bar(ref, classic))
    return ref


# ---- a. heads, forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,dtype,flags,sigma_only", INFERENCE_CASES)
def test_heads_forward_inference(probe, entry, dtype, flags, sigma_only):
    for name in sorted(PN.HEAD_SETS):
        what = "%s %#x flags %d %s" % (_ENTRY_NAMES[entry], dtype, flags, name)
        out = _forward(entry, dtype, flags, sigma_only, probe["rays"], probe["z"], probe["x"], PN.head_params(name))
        if sigma_only:
            _check_sigma(probe, out, name, ARITH[dtype & 0xff], False, what)
        else:
            _check_rgb(out[:, :3], name, bool(dtype & C), what)
            _check_sigma(probe, out[:, 3], name, ARITH[dtype & 0xff], False, what)


def _check_train_state(probe, dtype, out, acts, name, what):
    classic, state16 = bool(dtype & C), (dtype & 0xff) == STATE
    P = PN.N_RAYS * PN.N_SAMPLES
    o = out.cpu().numpy()
    ref = _check_rgb(o[:, :3], name, classic, what)
    _check_sigma(probe, o[:, 3], name, ARITH[dtype & 0xff], True, what)
    a = _state_np(acts, dtype)
    chans = list(ref["chans"])
    h2 = a[9, :P, :128].astype(np.float64)
    _note(what + " slot 9, probe channels", np.abs(h2[:, chans] - ref["h2"]), 0.0 if classic else PN.softplus_bar(ref["h2"], state16))
    rest = np.delete(h2, chans, 1)
    _note(what + " slot 9, other channels", np.abs(rest - ref["h2_rest"]), 0.0 if classic else PN.softplus_bar(ref["h2_rest"], state16))
    assert not a[8, :P].any(), what + ": slot 8 (xyz_encoding_final with zero weights) is not exactly 0"


@pytest.mark.parametrize("entry,dtype", TRAINING_CASES)
def test_heads_forward_and_backward_training(probe, entry, dtype):
    """a + b: the training forward's output and stored state, then the chain of the SAME dtype code (where the chain entry takes it) on the
    state that forward wrote, with a seeded normal g"""
    from sinnerf_amd import _lib
    chain_codes = {k[0] for k in _cases(CHAIN)}
    classic, state16 = bool(dtype & C), (dtype & 0xff) == STATE
    P = PN.N_RAYS * PN.N_SAMPLES
    g_np = np.random.RandomState(21).standard_normal((P, 4)).astype(np.float32)
    g = _t(g_np)
    for name in sorted(PN.HEAD_SETS):
        what = "%s %#x %s" % (_ENTRY_NAMES[entry], dtype, name)
        out, acts, emb = _train(entry, dtype, probe["rays"], probe["z"], probe["x"], PN.head_params(name))
        _check_train_state(probe, dtype, out, acts, name, what)
        if dtype not in chain_codes:           # SN_DTYPE_EMB_BF16 is not a chain dtype (the chain of the plain code reads the same state)
            continue
        rows = acts.shape[1]
        G = torch.full_like(acts, float("nan"))
        G[:, P:] = 0                           # the caller zero-fills the pad rows
        g_o = torch.full((P, 4), float("nan"), device=dev())
        arith = ARITH[dtype & 0xff]
        _lib.check(_lib.lib.sn_mlp_backward_chain(_lib.ptr(_model(arith).packed_bwd(arith)), dtype, _lib.ptr(acts), _lib.ptr(out), _lib.ptr(g), P, rows,
                                                  _lib.ptr(G), _lib.ptr(g_o), _lib.stream_ptr()), "sn_mlp_backward_chain")
        torch.cuda.synchronize()
        EXERCISED.add(_launcher(CHAIN, dtype, 0, 0, P))
        what = "chain %#x %s" % (dtype, name)
        ref = PN.head_reference(name, classic)
        g9 = (G[9, :P].float() if state16 else G[9, :P]).cpu().numpy().astype(np.float64)
        go = g_o.cpu().numpy()
        g64 = g_np.astype(np.float64)
        _note(what + " g_out rgb", np.abs(go[:, :3] - g64[:, :3] * ref["D3"]), PN.g_y3_bar(ref, g64[:, :3], classic))
        _note(what + " G[9][:, 128:131]", np.abs(g9[:, 128:131] - g64[:, :3] * ref["D3"]), PN.g_y3_bar(ref, g64[:, :3], classic, state16))
        assert np.array_equal(go[:, 3], g_np[:, 3]), what + ": g_out sigma"
        want = g[:, 3].bfloat16().float().cpu().numpy() if state16 else g_np[:, 3]
        assert np.array_equal(g9[:, 131].astype(np.float32), want), what + ": G[9][:, 131]"
        assert not g9[:, 132:160].any(), what + ": the head block's padding"
        chans = list(ref["chans"])
        g_y3 = go[:, :3].astype(np.float64)
        _note(what + " G[9][:, j]", np.abs(g9[:, chans] - ref["s"] * g_y3 * ref["D2"]), PN.g_y2_bar(ref, g_y3, classic, state16))
        assert not np.delete(g9[:, :128], chans, 1).any(), what + ": channels the rgb layer does not read"


# ---- c. embeddings ------------------------------------------------------------------------------------------------------------------------
def _emb_bar(arith):
    return PN.EMB_BAR_EXACT if arith in ("fp32", "bf16x3") else PN.EMB_BAR_DOUBLING


def _stored_embedding(emb, dtype, P):
    """the 63 + 27 reference columns of a stored embedding (fp32 form, or SN_DTYPE_EMB_BF16's K-slot order) as fp32 arrays"""
    if dtype & EMB:
        e = emb[:P].float().cpu().numpy()
        return e[:, [_emb_xyz_pos(c) for c in range(63)]], e[:, [64 + _emb_dir_pos(c) for c in range(27)]]
    e = emb[:P].cpu().numpy()
    return e[:, :63], e[:, 64:91]


_BIG = 40 * 256 + 77          # about 40 tiles: the persistent workgroups of the generated kernels walk more than one


@pytest.mark.parametrize("dtype,P", [(k[0], PN.N_RAYS * PN.N_SAMPLES) for k in _cases(TRAIN)] + [(F32, _BIG), (STATE, _BIG), (X3, _BIG)])
def test_stored_embedding_against_fp64_and_exact_points(dtype, P):
    """(i) rays whose origin is the probe point and whose depth is 0: every stored sin / cos column against fp64 of the exact fp32
    argument, |x| from 1e-3 to 1e3; (ii) general (o, d, z): the identity columns are the bits of fl(o + fl(d z)) -- a contracted FMA would
    move the top band by up to 0.03 rad at |x| = 1e3"""
    arith = ARITH[dtype & 0xff]
    half = (lambda r: PN.operand_half_ulp(r, "bf16")) if dtype & EMB else (lambda r: 0.0)
    o, d = PN.probe_values(P, 1), PN.probe_values(P, 2)
    rays = np.concatenate([o, d, np.zeros((P, 1), np.float32), np.ones((P, 1), np.float32)], 1)
    z = np.zeros((P, 1), np.float32)
    what = "train %#x P %d" % (dtype, P)
    out, acts, emb = _train(TRAIN, dtype, _t(rays), _t(z), None, PN.head_params("wide"))
    ex, ed = _stored_embedding(emb, dtype, P)
    rx, rd = PN.embedding64(o, 10), PN.embedding64(d, 4)
    _note(what + " stored Embedding(xyz)", np.abs(ex - rx), _emb_bar(arith) + half(rx))
    _note(what + " stored Embedding(dir)", np.abs(ed - rd), _emb_bar(arith) + half(rd))
    # (ii)
    rs = np.random.RandomState(6)
    rays[:, 0:3], rays[:, 3:6] = PN.probe_values(P, 3), PN.probe_values(P, 4)
    z = np.sort(10.0 ** rs.uniform(-3, 0, (P, 2)), -1).astype(np.float32)
    out, acts, emb = _train(TRAIN, dtype, _t(rays), _t(z), None)
    pts = O._points(rays, z).reshape(-1, 3)
    dirs = np.repeat(rays[:, 3:6], 2, 0)
    ex, ed = _stored_embedding(emb, dtype, 2 * P)
    if dtype & EMB:
        pts, dirs = _t(pts).bfloat16().float().cpu().numpy(), _t(dirs).bfloat16().float().cpu().numpy()
    assert np.array_equal(ex[:, :3], pts) and np.array_equal(ed[:, :3], dirs), what + ": identity columns"


@pytest.mark.parametrize("dtype,flags,sigma_only", RAY_FORWARD_CASES)
def test_inference_embedding_xyz_columns(dtype, flags, sigma_only):
    """(iii) the inference kernels do not store their embedding: the embedding probe turns sigma into column c, for all 63 columns"""
    arith = ARITH[dtype & 0xff]
    P = PN.N_RAYS * PN.N_SAMPLES
    o = PN.probe_values(P, 1)
    rays = _t(np.concatenate([o, PN.probe_values(P, 2), np.zeros((P, 1), np.float32), np.ones((P, 1), np.float32)], 1))
    z = _t(np.zeros((P, 1), np.float32))
    ref = PN.embedding64(o, 10)
    m = _model(arith, PN.embedding_params(0))
    w1 = m.xyz_encoding_1[0].weight
    err = np.zeros((P, 63))
    for c in range(63):
        with torch.no_grad():
            w1.zero_()
            w1[0, c], w1[1, c] = 1.0, -1.0
        out = _forward(FORWARD, dtype, flags, sigma_only, rays, z, None)
        err[:, c] = np.abs((out if sigma_only else out[:, 3]) - ref[:, c])
    bar = _emb_bar(arith) + PN.operand_half_ulp(ref, arith)
    what = "forward %#x flags %d sigma_only %d embedding probe" % (dtype, flags, sigma_only)
    _note(what + ", identity columns", err[:, :3], bar[:, :3])
    _note(what + ", sin / cos columns", err[:, 3:], bar[:, 3:])


@pytest.mark.parametrize("dtype,flags", sorted({k[:2] for k in _cases(FORWARD) if not k[2]}))
def test_inference_embedding_dir_columns(dtype, flags):
    """(iii) the 27 columns of Embedding(dir) through the head probe, y2 = a E_c + b: the rgb bar plus what the embedding's bar and the
    operand rounding of E_c (both times |a| <= 16), and the rounding of the sum y2, make of the colour through the two slopes"""
    arith, classic = ARITH[dtype & 0xff], bool(dtype & C)
    P = PN.N_RAYS * PN.N_SAMPLES
    d = PN.probe_values(P, 2)
    rays = _t(np.concatenate([PN.head_rays()[0][np.arange(P) % PN.N_RAYS, :3], d, np.zeros((P, 1), np.float32), np.ones((P, 1), np.float32)], 1))
    z = _t(np.ones((P, 1), np.float32))
    e64 = PN.embedding64(d, 4)
    a = np.abs(np.array(PN.HEAD_SETS["wide"][2], np.float64)[:, 0])
    worst = 0.0
    for c in range(27):
        out = _forward(FORWARD, dtype, flags, 0, rays, z, None, PN.dir_column_params("wide", c))
        ref = PN.head_reference("wide", classic, d_cols=np.repeat(e64[:, c:c + 1], 3, 1))
        y2_err = a * (_emb_bar(arith) + PN.operand_half_ulp(e64[:, c:c + 1], arith)) + PN.ulp32(ref["y2"])
        # both slopes are monotone, so their largest value within reach of the error sits at the end of the interval
        with np.errstate(over="ignore"):
            slope2 = (ref["y2"] + y2_err > 0).astype(np.float64) if classic else 1.0 / (1.0 + np.exp(-(ref["y2"] + y2_err - 1.0)))
        reach = np.abs(ref["s"]) * slope2 * y2_err
        y3_near = np.maximum(np.abs(ref["y3"]) - reach, 0.0)
        slope3 = np.exp(-y3_near) / (1.0 + np.exp(-y3_near)) ** 2 if classic else 0.25 * PN._SCALE * (1.0 - np.tanh(0.5 * y3_near) ** 2)
        bar = PN.rgb_bar(ref, classic) + reach * slope3
        err = np.abs(out[:, :3] - ref["rgb"])
        assert np.isfinite(err).all()
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (hex(dtype), flags, c, float((err / bar).max()))
    WORST["forward %#x flags %d dir columns" % (dtype, flags)] = worst
    print("forward %#x flags %d, 27 dir columns through the head probe: worst err / bar %.3f" % (dtype, flags, worst))


def test_zz_every_exported_launcher_was_exercised():
    """runs last in the module: the launchers the tests above handed work to are all 32 the library exports"""
    import re
    import subprocess
    from sinnerf_amd import _lib
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(sn_mlp_(?:forward|backward_chain)_\w+)_launch\b", syms))
    fwd = {s for s in exported if s.startswith("sn_mlp_forward")}
    assert len(exported) == 32 and len(fwd) == 20, sorted(exported)
    for k in sorted(WORST):
        print("%-70s %.3f" % (k, WORST[k]))
    assert EXERCISED == exported, (sorted(exported - EXERCISED), sorted(EXERCISED - exported))
