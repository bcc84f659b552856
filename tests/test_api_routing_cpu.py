"""Which kernel an MLP entry of the C ABI runs, and which error code it refuses a call with: host logic of csrc/sn_api.hip, checked without
a GPU.  The GPU tests compare kernel generations bit for bit -- a router that sent SN_DTYPE_COMPILER_SCHEDULED or SN_FLAG_F32_LDS_RING to the
default kernel would make them compare a kernel with itself -- so the routing is pinned here, through the introspection entry
``sn_mlp_route``, against a literal table written from the if-chains the router replaced.

The library is loaded with ctypes directly (not through ``sinnerf_amd._lib``, which resolves every declared symbol): the refusal test
also has to pass against an older build of the same ABI named by SINNERF_HIP_LIB."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SINNERF_HIP_LIB") or os.path.join(REPO, "sinnerf_amd", "csrc", "libsinnerf_hip.so")

F32, BF16, STATE, X3, F16 = 0, 1, 2, 3, 4                    # SN_DTYPE_*
C, PREV, EMB = 0x100, 0x200, 0x400                           # SN_DTYPE_CLASSIC_HEADS, _COMPILER_SCHEDULED, _EMB_BF16
BF16_CS, RING = 2, 4                                         # SN_FLAG_BF16_COMPILER_SCHEDULED, SN_FLAG_F32_LDS_RING
FORWARD, FORWARD_EMBEDDED, TRAIN, TRAIN_EMBEDDED, CHAIN = range(5)      # SN_ROUTE_*
LO, HI = 2 ** 31 - 257, 2 ** 31 - 256                        # the generated training kernels index points with 32 bits: LO is their last size
E_BADARG, E_UNSUPPORTED, E_BADSHAPE = -1, -4, -5


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(LIB_PATH)
    vp, i, l_ = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    for name, args in (("sn_mlp_forward", [vp, i, vp, vp, l_, i, i, i, vp, vp]),
                       ("sn_mlp_forward_embedded", [vp, i, vp, l_, i, i, i, vp, vp]),
                       ("sn_mlp_forward_train", [vp, i, vp, vp, l_, i, vp, vp, vp, l_, vp]),
                       ("sn_mlp_forward_train_embedded", [vp, i, vp, l_, i, vp, vp, l_, vp]),
                       ("sn_mlp_backward_chain", [vp, i, vp, vp, vp, l_, l_, vp, vp, vp])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = i, args
    return lib


# (dtype, flags, sigma_only, n_points) -> launcher symbol without "sn_mlp_" in front and "_launch" behind; None = the entry refuses the dtype
ROUTES = {
    FORWARD: [
        ((F32, 0, 0, 1000), "forward_f32g"), ((F32, 0, 1, 1000), "forward_f32g"),
        ((F32 | C, 0, 0, 1000), "forward_f32g_classic"), ((F32 | C, 0, 1, 1000), "forward_f32g"),
        ((F32, RING, 0, 1000), "forward_f32"), ((F32, RING, 1, 1000), "forward_f32"),
        ((F32 | C, RING, 0, 1000), "forward_f32_classic"), ((F32 | C, RING, 1, 1000), "forward_f32"),
        ((F32, BF16_CS, 0, 1000), "forward_f32g"), ((F32, RING | BF16_CS, 0, 1000), "forward_f32"),
        ((BF16, 0, 0, 1000), "forward_bf16_v3"), ((BF16, 0, 1, 1000), "forward_bf16"),
        ((BF16 | C, 0, 0, 1000), "forward_bf16_v3_classic"), ((BF16 | C, 0, 1, 1000), "forward_bf16"),
        ((BF16, BF16_CS, 0, 1000), "forward_bf16"), ((BF16, BF16_CS, 1, 1000), "forward_bf16"),
        ((BF16 | C, BF16_CS, 0, 1000), "forward_bf16_classic"), ((BF16 | C, BF16_CS, 1, 1000), "forward_bf16"),
        ((BF16, RING, 0, 1000), "forward_bf16_v3"), ((BF16, 1 | 8, 0, 1000), "forward_bf16_v3"),
        ((F16, 0, 0, 1000), "forward_bf16_v3_f16"), ((F16, 0, 1, 1000), "forward_bf16_f16"),
        ((F16 | C, 0, 0, 1000), "forward_bf16_v3_f16_classic"), ((F16 | C, 0, 1, 1000), "forward_bf16_f16"),
        ((F16, BF16_CS, 0, 1000), "forward_bf16_f16"), ((F16 | C, BF16_CS, 0, 1000), "forward_bf16_f16_classic"),
        ((X3, 0, 0, 1000), "forward_bf16x3"), ((X3, 0, 1, 1000), "forward_bf16x3"),
        ((X3 | C, 0, 0, 1000), "forward_bf16x3_classic"), ((X3 | C, 0, 1, 1000), "forward_bf16x3"),
        ((X3, RING | BF16_CS, 0, 1000), "forward_bf16x3"), ((X3, 0, 0, HI), "forward_bf16x3"),
        ((STATE, 0, 0, 1000), None), ((7, 0, 0, 1000), None), ((-1, 0, 0, 1000), None),
        ((BF16 | PREV, 0, 0, 1000), None), ((BF16 | C | PREV, 0, 0, 1000), None), ((F32 | EMB, 0, 0, 1000), None),
    ],
    FORWARD_EMBEDDED: [
        ((F32, 0, 0, 1000), "forward_f32g"), ((F32, 0, 1, 1000), "forward_f32g"),
        ((F32 | C, 0, 0, 1000), "forward_f32g_classic"), ((F32 | C, 0, 1, 1000), "forward_f32g"),
        ((F32, RING, 0, 1000), "forward_f32"), ((F32, RING, 1, 1000), "forward_f32"),
        ((F32 | C, RING, 0, 1000), "forward_f32_classic"), ((F32 | C, RING, 1, 1000), "forward_f32"),
        ((BF16, 0, 0, 1000), "forward_bf16"), ((BF16, 0, 1, 1000), "forward_bf16"),          # the hand-scheduled kernel takes rays only
        ((BF16 | C, 0, 0, 1000), "forward_bf16_classic"), ((BF16 | C, 0, 1, 1000), "forward_bf16"),
        ((BF16, BF16_CS, 0, 1000), "forward_bf16"), ((BF16 | C, BF16_CS, 0, 1000), "forward_bf16_classic"),
        ((F16, 0, 0, 1000), "forward_bf16_f16"), ((F16, 0, 1, 1000), "forward_bf16_f16"),
        ((F16 | C, 0, 0, 1000), "forward_bf16_f16_classic"), ((F16 | C, 0, 1, 1000), "forward_bf16_f16"),
        ((X3, 0, 0, 1000), "forward_bf16x3"), ((X3, 0, 1, 1000), "forward_bf16x3"),
        ((X3 | C, 0, 0, 1000), "forward_bf16x3_classic"), ((X3 | C, 0, 1, 1000), "forward_bf16x3"),
        ((STATE, 0, 0, 1000), None), ((5, 0, 0, 1000), None), ((F32 | PREV, 0, 0, 1000), None), ((F32 | C | EMB, 0, 0, 1000), None),
    ],
    TRAIN: [
        ((F32, 0, 0, 1000), "forward_f32g_store"), ((F32 | C, 0, 0, 1000), "forward_f32g_store_classic"),
        ((F32, 0, 0, HI), "forward_f32g_store"),
        ((F32 | PREV, 0, 0, 1000), "forward_f32"), ((F32 | PREV | C, 0, 0, 1000), "forward_f32_classic"),
        ((F32 | PREV, RING, 1, 1000), "forward_f32"),                                        # flags / sigma_only: not arguments of this entry
        ((F32 | EMB, 0, 0, 1000), None), ((F32 | EMB | C, 0, 0, 1000), None),
        ((BF16, 0, 0, 1000), "forward_bf16"), ((BF16 | C, 0, 0, 1000), "forward_bf16_classic"),
        ((BF16 | PREV, 0, 0, 1000), "forward_bf16"), ((BF16 | PREV | C, 0, 0, 1000), "forward_bf16_classic"),
        ((BF16 | EMB, 0, 0, 1000), None),
        ((STATE, 0, 0, 1000), "forward_bf16_t"), ((STATE | C, 0, 0, 1000), "forward_bf16_t_classic"),
        ((STATE, 0, 0, LO), "forward_bf16_t"), ((STATE, 0, 0, HI), "forward_bf16"),
        ((STATE | C, 0, 0, LO), "forward_bf16_t_classic"), ((STATE | C, 0, 0, HI), "forward_bf16_classic"),
        ((STATE | PREV, 0, 0, 1000), "forward_bf16"), ((STATE | PREV | C, 0, 0, 1000), "forward_bf16_classic"),
        ((STATE | EMB, 0, 0, 1000), "forward_bf16_t"), ((STATE | EMB | C, 0, 0, 1000), "forward_bf16_t_classic"),
        ((STATE | EMB, 0, 0, LO), "forward_bf16_t"), ((STATE | EMB, 0, 0, HI), None),
        ((STATE | EMB | PREV, 0, 0, 1000), None), ((STATE | EMB | PREV | C, 0, 0, 1000), None),
        ((X3, 0, 0, 1000), "forward_bf16x3_t"), ((X3 | C, 0, 0, 1000), "forward_bf16x3_t_classic"),
        ((X3, 0, 0, LO), "forward_bf16x3_t"), ((X3, 0, 0, HI), "forward_bf16x3"),
        ((X3 | C, 0, 0, LO), "forward_bf16x3_t_classic"), ((X3 | C, 0, 0, HI), "forward_bf16x3_classic"),
        ((X3 | PREV, 0, 0, 1000), "forward_bf16x3"), ((X3 | PREV | C, 0, 0, 1000), "forward_bf16x3_classic"),
        ((X3 | EMB, 0, 0, 1000), None), ((X3 | EMB | C, 0, 0, 1000), None),
        ((F16, 0, 0, 1000), None), ((F16 | C, 0, 0, 1000), None), ((6, 0, 0, 1000), None), ((F32 | 0x800, 0, 0, 1000), None),
    ],
    TRAIN_EMBEDDED: [
        ((F32, 0, 0, 1000), "forward_f32g_store"), ((F32 | C, 0, 0, 1000), "forward_f32g_store_classic"),
        ((STATE, 0, 0, 1000), "forward_bf16"), ((STATE | C, 0, 0, 1000), "forward_bf16_classic"),      # the generated kernels take rays only
        ((STATE, 0, 0, LO), "forward_bf16"), ((STATE, 0, 0, HI), "forward_bf16"),
        ((X3, 0, 0, 1000), "forward_bf16x3"), ((X3 | C, 0, 0, 1000), "forward_bf16x3_classic"),
        ((X3, 0, 0, LO), "forward_bf16x3"), ((X3, 0, 0, HI), "forward_bf16x3"),
        ((BF16, 0, 0, 1000), None), ((BF16 | C, 0, 0, 1000), None), ((F16, 0, 0, 1000), None),
        ((F32 | PREV, 0, 0, 1000), None), ((F32 | PREV | C, 0, 0, 1000), None), ((STATE | EMB, 0, 0, 1000), None),
    ],
    CHAIN: [
        ((F32, 0, 0, 1000), "backward_chain_f32g"), ((F32 | C, 0, 0, 1000), "backward_chain_f32g_classic"),
        ((F32, 0, 0, HI), "backward_chain_f32g"),
        ((F32 | PREV, 0, 0, 1000), "backward_chain_f32"), ((F32 | PREV | C, 0, 0, 1000), "backward_chain_f32_classic"),
        ((BF16, 0, 0, 1000), "backward_chain_bf16"), ((BF16 | C, 0, 0, 1000), "backward_chain_bf16_classic"),
        ((BF16 | PREV, 0, 0, 1000), "backward_chain_bf16"), ((BF16 | PREV | C, 0, 0, 1000), "backward_chain_bf16_classic"),
        ((STATE, 0, 0, 1000), "backward_chain_bf16_t"), ((STATE | C, 0, 0, 1000), "backward_chain_bf16_t_classic"),
        ((STATE, 0, 0, LO), "backward_chain_bf16_t"), ((STATE, 0, 0, HI), "backward_chain_bf16"),
        ((STATE | C, 0, 0, LO), "backward_chain_bf16_t_classic"), ((STATE | C, 0, 0, HI), "backward_chain_bf16_classic"),
        ((STATE | PREV, 0, 0, 1000), "backward_chain_bf16"), ((STATE | PREV | C, 0, 0, 1000), "backward_chain_bf16_classic"),
        ((STATE, RING, 1, 1000), "backward_chain_bf16_t"),                                   # flags / sigma_only: not arguments of this entry
        ((X3, 0, 0, 1000), "backward_chain_bf16x3_t"), ((X3 | C, 0, 0, 1000), "backward_chain_bf16x3_t_classic"),
        ((X3, 0, 0, LO), "backward_chain_bf16x3_t"), ((X3, 0, 0, HI), "backward_chain_bf16x3"),
        ((X3 | C, 0, 0, LO), "backward_chain_bf16x3_t_classic"), ((X3 | C, 0, 0, HI), "backward_chain_bf16x3_classic"),
        ((X3 | PREV, 0, 0, 1000), "backward_chain_bf16x3"), ((X3 | PREV | C, 0, 0, 1000), "backward_chain_bf16x3_classic"),
        ((F16, 0, 0, 1000), None), ((STATE | EMB, 0, 0, 1000), None), ((STATE | EMB | C, 0, 0, 1000), None), ((9, 0, 0, 1000), None),
    ],
}


def test_routing_table(lib):
    lib.sn_mlp_route.restype = ctypes.c_char_p
    lib.sn_mlp_route.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long]
    # the three rows a router that forgot a previous-generation bit would get wrong
    assert ((F32 | PREV, 0, 0, 1000), "forward_f32") in ROUTES[TRAIN]
    assert ((F32, RING, 0, 1000), "forward_f32") in ROUTES[FORWARD]
    assert ((X3 | PREV, 0, 0, 1000), "forward_bf16x3") in ROUTES[TRAIN] and ((X3 | PREV, 0, 0, 1000), "backward_chain_bf16x3") in ROUTES[CHAIN]
    wrong = []
    for entry, rows in ROUTES.items():
        for (dtype, flags, sigma_only, n_points), want in rows:
            got = lib.sn_mlp_route(entry, dtype, flags, sigma_only, n_points)
            got = got.decode() if got is not None else None
            if got != (None if want is None else "sn_mlp_" + want):
                wrong.append((entry, hex(dtype), flags, sigma_only, n_points, want, got))
            if sigma_only and entry in (FORWARD, FORWARD_EMBEDDED):
                assert got is None or not got.endswith("_classic"), (entry, hex(dtype), flags, got)      # never reaches the heads
    assert not wrong, wrong
    assert lib.sn_mlp_route(-1, F32, 0, 0, 1000) is None and lib.sn_mlp_route(5, F32, 0, 0, 1000) is None
    # every MLP launcher the library exports is the answer of at least one row, and every answer is an exported launcher
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(sn_mlp_(?:forward|backward_chain)_\w+)_launch\b", syms))
    routed = {"sn_mlp_" + want for rows in ROUTES.values() for _, want in rows if want is not None}
    assert len(exported) == 32, sorted(exported)             # 16 kernel files / operand passes x the two head passes
    assert routed == exported, (sorted(exported - routed), sorted(routed - exported))


def test_refusal_codes(lib):
    """Argument combinations every entry refuses before it touches the device (nothing here reaches a launcher): the code, and which code
    wins where several apply, are part of the ABI."""
    p = 0x1000                                               # a fake non-null device pointer: never dereferenced on these paths
    fwd = lambda dtype, blob=p, n_rays=4, n_samples=8, sigma_only=0: lib.sn_mlp_forward(blob, dtype, p, p, n_rays, n_samples, sigma_only, 0, p, None)
    emb = lambda dtype, ld, sigma_only=0, x=p: lib.sn_mlp_forward_embedded(p, dtype, x, 32, ld, sigma_only, 0, p, None)
    train = lambda dtype, slot_rows, n_rays=4, n_samples=64, acts=p: lib.sn_mlp_forward_train(p, dtype, p, p, n_rays, n_samples, p, acts, p, slot_rows, None)
    train_e = lambda dtype, ld, slot_rows=256, out=p: lib.sn_mlp_forward_train_embedded(p, dtype, p, 32, ld, out, p, slot_rows, None)
    chain = lambda dtype, slot_rows, n_points=256, g_out=p: lib.sn_mlp_backward_chain(p, dtype, p, p, p, n_points, slot_rows, p, g_out, None)
    cases = [
        # a null pointer
        ("forward: null blob", fwd(F32, blob=None), E_BADARG),
        ("forward_embedded: null x", emb(F32, 90, x=None), E_BADARG),
        ("train: null acts", train(F32, 256, acts=None), E_BADARG),
        ("train_embedded: null out", train_e(F32, 90, out=None), E_BADARG),
        ("chain: null g_out", chain(F32, 256, g_out=None), E_BADARG),
        ("chain: null g_out wins over a bad dtype", chain(7, 256, g_out=None), E_BADARG),
        # sn_mlp_forward
        ("forward: n_samples 0", fwd(F32, n_samples=0), E_BADARG),
        ("forward: dtype 2", fwd(STATE), E_UNSUPPORTED),
        ("forward: dtype 1 | 0x200", fwd(BF16 | PREV), E_UNSUPPORTED),
        ("forward: dtype 7", fwd(7), E_UNSUPPORTED),
        ("forward: dtype 7 | classic, sigma-only", fwd(7 | C, sigma_only=1), E_UNSUPPORTED),
        # sn_mlp_forward_train: arguments, base dtype, slot_rows, then the SN_DTYPE_EMB_BF16 refusal
        ("train: F16", train(F16, 256), E_UNSUPPORTED),
        ("train: F16 with short slot_rows", train(F16, 0), E_UNSUPPORTED),
        ("train: F32, slot_rows one tile short", train(F32, 128), E_BADSHAPE),
        ("train: F32 | EMB_BF16, short slot_rows", train(F32 | EMB, 128), E_BADSHAPE),
        ("train: F32 | EMB_BF16, adequate slot_rows", train(F32 | EMB, 256), E_UNSUPPORTED),
        ("train: STATE | EMB_BF16 | COMPILER_SCHEDULED", train(STATE | EMB | PREV, 256), E_UNSUPPORTED),
        ("train: BF16X3 | EMB_BF16, slot_rows % 128 != 0", train(X3 | EMB, 264), E_UNSUPPORTED),
        ("train: BF16X3, slot_rows % 128 != 0", train(X3, 264), E_BADSHAPE),
        ("train: BF16_STATE, 129 points, slot_rows 128", train(STATE, 128, n_rays=1, n_samples=129), E_BADSHAPE),
        # sn_mlp_forward_train_embedded: ld before the dtype
        ("train_embedded: ld 89 with a bad dtype", train_e(BF16, 89), E_BADSHAPE),
        ("train_embedded: dtype 1", train_e(BF16, 90), E_UNSUPPORTED),
        ("train_embedded: F32 | 0x200", train_e(F32 | PREV, 90), E_UNSUPPORTED),
        ("train_embedded: F32, slot_rows short", train_e(F32, 90, slot_rows=16), E_BADSHAPE),
        # sn_mlp_backward_chain
        ("chain: EMB_BF16", chain(STATE | EMB, 256), E_UNSUPPORTED),
        ("chain: F16", chain(F16, 256), E_UNSUPPORTED),
        ("chain: BF16X3, slot_rows % 128 != 0", chain(X3, 264), E_BADSHAPE),
        ("chain: BF16_STATE, slot_rows one 128 short of a 256-point tile", chain(STATE, 384, n_points=257), E_BADSHAPE),
        # sn_mlp_forward_embedded
        ("forward_embedded: ld 62 sigma-only", emb(F32, 62, sigma_only=1), E_BADSHAPE),
        ("forward_embedded: ld 89 with heads", emb(F32, 89), E_BADSHAPE),
        ("forward_embedded: ld 89 with heads and a bad dtype", emb(STATE, 89), E_BADSHAPE),
        ("forward_embedded: dtype 2", emb(STATE, 90), E_UNSUPPORTED),
    ]
    wrong = [(what, got, want) for what, got, want in cases if got != want]
    assert not wrong, wrong
