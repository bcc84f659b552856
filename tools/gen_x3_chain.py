#!/usr/bin/env python3
"""Generator of the hand-scheduled slab loop of the bf16x3 backward chain (sinnerf_amd/csrc/sn_mlp_bwd_bf16x3_t.hip).

The chain = input-gradient propagation g_x = W^T g_y, g_y = g_h (.) act'(.) through dir_encoding^T, xyz_encoding_final^T and
xyz_encoding_8..2^T -- what torch autograd derives from models/nerf.py:122-148 -- for one wave's ONE 32-point tile in the 3-term split
arithmetic of csrc/sn_mlp_x3.h (W^T g ~= Wh^T gh + Wl^T gh + Wh^T gl on v_mfma_f32_32x32x16_bf16, two accumulator chains in strict
alternation A B A | B A B, both started from the literal 0): the 72 transposed (hi, lo) weight slabs of csrc/sn_layout.h
("Backward-chain blob, bf16x3"), 3 264 MFMAs.  Same arithmetic and accumulation order, same stored gradient state (G slots 0..8 as
(hi, lo) pairs) as the compiler-scheduled mlp_bwd_chain_bf16x3_kernel it replaces (bit-identical on the device), laid out by the list
scheduler of tools/mfma_stream.py like the training forward (tools/gen_x3_trunk.py); executed on the CPU by
tools/gcn_sim.py (tests/test_streams_cpu.py).

Per output tile (slab s = tile t of chain layer L) the deferred epilogue, run inside slab s + 1, per block of four accumulator registers:
  x = A + B (v_add_f32); [xyz_encoding_final^T: the sigma head's term x += sigma.weight[f] g_sigma (nerf.py:136), v_fmac_f32];
  [ReLU mask from the SIGN WORD the training forward left for this (layer, tile pair): v_bfe_i32 + v_and_b32 per value]; hi = cvt_pk(v)
  -> AGPRs of the other activation set; lo = cvt_pk(v - float(hi)) -> AGPRs; two v_permlane32_swap_b32 + ONE ds_write_b128 into the
  wave's staging tile (32 rows x 128 B, chunk ^= row & 7: conflict-free both ways); then the tile's row stores: 4 x (ds_read_b128 +
  global_store_dwordx4 nt of 8 whole 128-byte point segments of G[slot]).
Sign words: the 8 x 4 words of a point tile are loaded by the kernel in front of the statement (eight 16-byte loads per lane) and
handed in as operands -- no load inside the slab loop (the compiler-scheduled kernel requested each layer's words a layer ahead and
took them over with a hand-counted vmcnt).
Weight ring: FOUR slots of 32 KB (the widest transposed slab; the chain has no bias table in front of the ring to make room for),
slab s in slot s % 4 (72 = 0 mod 4: static), staged 3 slabs ahead behind ONE sync point per slab (counted vmcnt for slab s + 1 derived
from the emitted order, then the barrier, then the pieces of slab s + 3); slabs 69..71 stage the next point tile's slabs 0..2 (the
stream wraps).

Register plan inside the statement (v[128:255] named as clobbers; the kernel keeps v0..v127, where the sign words live):
  v[128:191] accumulators [set][chain][16]     v[192:223] A-fragment ring: 4 entries x (hi 4 + lo 4)
  v[224:227] sigma^T weights of the block in flight    v[228:231], v[232:235] row buffers    v[236:237] float(hi) temporaries
  s[84:85] running pointer into G[slot] (- slot_rows * 1024 B per layer)

usage: gen_x3_chain.py out.inc [knob=value ...]
"""
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfma_stream as S                         # noqa: E402  (Emitter, Backbone, Scheduler, Filler, write_inc)

KNOBS = dict(prefetch=3, cap=5.0, dma_cost=2.0, valu_cost=1.0, lds_cost=1.0, salu_cost=0.5,
             bar_gap=3,         # the sync point sits behind this MFMA of a slab
             epi_from=1,
             pk=0)              # 1: v_pk_add_f32 (see tools/gen_x3_trunk.py: an anti-lever beside MFMAs)

N_SLABS = 72
N_SLOTS, SLOT_BYTES, DMA_DIST = 4, 32768, 3
ACC = lambda st, ch: 128 + st * 32 + ch * 16
RING0, RING_N = 192, 4
SIGT = 224
ROW_A, ROW_B = 228, 232
TMP0 = 236
SGPR_G = 84


def nk_of(s): return 8 if s < 8 else 16
def layer_of(s): return s // 8                # 0 dir_encoding^T, 1 xyz_encoding_final^T, L >= 2: xyz_encoding_{10 - L}^T
def slab_bytes(s): return nk_of(s) * 2048
def read_set(L): return L & 1
def write_set(L): return 1 - (L & 1)
def out_slot(L): return 8 if L == 0 else 8 - L            # G slot the layer writes = acts slot of its ReLU mask (L >= 1)
def x3_reg(st, part, ks): return st * 128 + part * 64 + ks * 4
def ring(kidx): return RING0 + 8 * (kidx % RING_N)
TOTAL_BYTES = sum(slab_bytes(s) for s in range(N_SLABS))


def plan(K):
    P = SimpleNamespace(K=K, D=K["prefetch"])
    assert 1 <= P.D <= RING_N - 1
    P.bb = S.Backbone(N_SLABS, nk_of, 3)          # mf[i] = (slab, k-step, term) as in gen_x3_trunk.py
    P.bar = {s: P.bb.first[s] + K["bar_gap"] - 1 for s in range(N_SLABS)}
    return P


def frag_read(P, kidx, part):
    s, ks = P.bb.kstep_list[kidx]
    slot, r = s % N_SLOTS, ring(kidx) + 4 * part
    return "ds_read_b128 v[%d:%d], %s offset:%d" % (r, r + 3, ("%[vaA]", "%[vaB]")[slot >> 1], (slot & 1) * SLOT_BYTES + ks * 2048 + part * 1024)


def add_fragments(P, sched):
    """A fragments (the first D k-steps are loaded in the preamble: slab 0 is resident)"""
    D, idx_of, ksl = P.D, P.bb.idx_of, P.bb.kstep_list
    for kidx in range(D, len(ksl)):
        s, ks = ksl[kidx]
        prev_user = idx_of[ksl[kidx - RING_N] + (2,)] if kidx >= RING_N else -1
        rel = max(prev_user, idx_of[ksl[kidx - D] + (0,)])
        if s > 0:
            rel = max(rel, P.bar[s - 1] + 1)                         # the sync point of slab s - 1 makes slab s visible
        for part in range(2):
            sched.add(S.Filler(frag_read(P, kidx, part), P.K["lds_cost"], rel, idx_of[(s, ks, 0)] - 1, "ds_read", tag=("frag", kidx, part)))


def epilogue(K, s):
    """epilogue of slab s (tile t of chain layer L), run inside slab s + 1: the blocks, then the tile's row stores"""
    L, t = layer_of(s), s % 8
    W, st = write_set(L), s & 1
    copy, sig = L == 0, L == 1
    items = []
    V = lambda text, writes=(), tag=None: items.append(("valu", text, writes, tag, "acc"))
    for i in range(4):
        a, b = ACC(st, 0) + 4 * i, ACC(st, 1) + 4 * i
        rh = x3_reg(W, 0, 2 * t + (i >> 1)) + 2 * (i & 1)
        rl = x3_reg(W, 1, 2 * t + (i >> 1)) + 2 * (i & 1)
        if sig:
            items.append(("ds_read", "ds_read_b128 v[%d:%d], %%[vs] offset:%d" % (SIGT, SIGT + 3, (16 * t + 4 * i) * 4), (), ("sigt", s, i), "acc"))
        if K["pk"]:
            V("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (a, a + 1, a, a + 1, b, b + 1), (a, a + 1))
            V("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (a + 2, a + 3, a + 2, a + 3, b + 2, b + 3), (a + 2, a + 3))
        else:
            for e in range(4):
                V("v_add_f32 v%d, v%d, v%d" % (a + e, a + e, b + e), (a + e,))
        if sig:                                                  # x += sigma.weight[f] * g_sigma  (fused, as __builtin_fmaf in the C++ kernel)
            for e in range(4):
                V("v_fmac_f32 v%d, v%d, %%[gsig]" % (a + e, SIGT + e), (a + e,), ("sigt", s, i))
        if not copy:                                             # g_y = g_h [h > 0]: bit k <- value 0, 16 + k <- value 1, k + 1 / 17 + k <- values 2 / 3
            k = 2 * i + 8 * (t & 1)
            word = "%%[sw%d_%d]" % (out_slot(L), t >> 1)
            for e, bit in enumerate((k, k + 16, k + 1, k + 17)):
                V("v_bfe_i32 v%d, %s, %d, 1" % (b + e, word, bit), (b + e,))
            for e in range(4):
                V("v_and_b32 v%d, v%d, v%d" % (a + e, b + e, a + e), (a + e,))
        V("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (b, a, a + 1), (b,))
        V("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (b + 1, a + 2, a + 3), (b + 1,))
        V("v_accvgpr_write_b32 a%d, v%d" % (rh, b), (("a", rh),))
        V("v_accvgpr_write_b32 a%d, v%d" % (rh + 1, b + 1), (("a", rh + 1),))
        for half in range(2):
            V("v_lshlrev_b32 v%d, 16, v%d" % (TMP0, b + half), (TMP0,))
            V("v_and_b32 v%d, 0xffff0000, v%d" % (TMP0 + 1, b + half), (TMP0 + 1,))
            x = a + 2 * half
            if K["pk"]:
                V("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d] neg_lo:[0,1] neg_hi:[0,1]" % (x, x + 1, x, x + 1, TMP0, TMP0 + 1), (x, x + 1))
            else:
                V("v_sub_f32 v%d, v%d, v%d" % (x, x, TMP0), (x,))
                V("v_sub_f32 v%d, v%d, v%d" % (x + 1, x + 1, TMP0 + 1), (x + 1,))
        V("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (b + 2, a, a + 1), (b + 2,))
        V("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (b + 3, a + 2, a + 3), (b + 3,))
        V("v_accvgpr_write_b32 a%d, v%d" % (rl, b + 2), (("a", rl),))
        V("v_accvgpr_write_b32 a%d, v%d" % (rl + 1, b + 3), (("a", rl + 1),))
        items.append(("swap", "v_permlane32_swap_b32 v%d, v%d" % (b, b + 2), (b, b + 2), None, "acc", (b, b + 2)))
        items.append(("swap", "v_permlane32_swap_b32 v%d, v%d" % (b + 1, b + 3), (b + 1, b + 3), None, "acc", (b + 1, b + 3)))
        items.append(("ds_write", "ds_write_b128 %%[stw%d], v[%d:%d]" % (i, b, b + 3), (), None, "acc"))
    rows = []
    def rd(n):
        ro = ROW_B if n & 1 else ROW_A
        rows.append(("ds_read", "ds_read_b128 v[%d:%d], %%[str] offset:%d" % (ro, ro + 3, 1024 * n), (), ("ro", s, n), "post"))
    def st_(n):
        ro = ROW_B if n & 1 else ROW_A
        rows.append(("vstore", "global_store_dwordx4 %%[vo], v[%d:%d], s[%d:%d] offset:%d nt" % (ro, ro + 3, SGPR_G, SGPR_G + 1, 128 * t),
                     (), ("ro", s, n), "post", (SGPR_G, SGPR_G + 1)))
        if n < 3:
            rows.append(("valu", "v_add_u32 %[vo], 8192, %[vo]", ("vo",), None, "post"))
        else:
            rows.append(("valu", "v_subrev_u32 %[vo], 24576, %[vo]", ("vo",), None, "post"))
    rd(0); rd(1)
    for n in range(4):
        st_(n)
        if n + 2 < 4:
            rd(n + 2)
    if t == 7 and L < 8:                                         # next layer: G[slot - 1]
        rows.append(("salu", "s_sub_u32 s%d, s%d, %%[srlo]" % (SGPR_G, SGPR_G), (SGPR_G,), None, "post"))
        rows.append(("salu", "s_subb_u32 s%d, s%d, %%[srhi]" % (SGPR_G + 1, SGPR_G + 1), (SGPR_G + 1,), None, "post"))
    return items + rows


def add_weight_stream(P, sched):
    """sync point + weight stream: slab s + 1 awaited, then the pieces of slab s + 3 (s >= 69: the next point tile's slabs 0..2)"""
    first, bar = P.bb.first, P.bar
    for s in range(N_SLABS):
        sched.add(S.Filler("", 0.5, bar[s], bar[s], "bar", tag=s + 1))
        tgt = s + DMA_DIST
        real = tgt % N_SLABS
        pieces = slab_bytes(real) // 4096
        stride = max(1, (first[s + 1] - 2 - bar[s] - 1) // pieces)
        dl = first[s + 1] - 1
        for p in range(pieces):
            wrap = tgt >= N_SLABS and real == 0 and p == 0               # the stream wraps: back to the start of the blob
            sched.weight_stream_piece("s_add_u32 m0, %%[sm], %d" % ((real % N_SLOTS) * SLOT_BYTES + p * 4096),
                                      min(bar[s] + 1 + p * stride, dl), dl, tgt, rewind=TOTAL_BYTES if wrap else None)


def preamble(P, g):
    for dst, src in ((SGPR_G, "gplo"), (SGPR_G + 1, "gphi")):
        g.salu_mov(dst, "%%[%s]" % src)
    for kidx in range(P.D):
        for part in range(2):
            g.ds_read(frag_read(P, kidx, part), ("frag", kidx, part))


def issue_mfma(P, g, entry):
    s, ks, term = entry
    kidx = P.bb.gk[(s, ks)]
    if term == 0:
        g.wait_lgkm({("frag", kidx, 0), ("frag", kidx, 1)})      # one counted wait per k-step (the lo read follows the hi read)
    c0, c1 = (0, 1) if (ks & 1) == 0 else (1, 0)
    d = ACC(s & 1, c1 if term == 1 else c0)
    c_txt = "0" if (ks == 0 and term <= 1) else "v[%d:%d]" % (d, d + 15)      # both chains start from zero (no bias in the chain)
    b0 = x3_reg(read_set(layer_of(s)), 1 if term == 2 else 0, ks)
    g.pad_valu_to_mfma([("a", b0 + e) for e in range(4)])
    a_reg = ring(kidx) + (4 if term == 1 else 0)
    g.mfma("v_mfma_f32_32x32x16_bf16 v[%d:%d], v[%d:%d], a[%d:%d], %s" % (d, d + 15, a_reg, a_reg + 3, b0, b0 + 3, c_txt))


def gen(knobs):
    K, P = knobs, plan(knobs)
    g = S.Emitter([1] * 4 + [2] * 4)              # entry: at most the pieces of slabs 1, 2 in flight
    sched = S.Scheduler(g, K["dma_cost"], K["valu_cost"], K["lds_cost"], K["salu_cost"])
    add_fragments(P, sched)
    def handover(s):                              # the next layer's first slab reads k-steps 14, 15 of the written set
        if s % 8 == 7 and layer_of(s) + 1 <= 8:
            return P.bb.idx_of[(s + 1, 14, 0)]
    epi_tail = sched.add_deferred_epilogues(P.bb, lambda s: epilogue(K, s), K["epi_from"], handover)
    add_weight_stream(P, sched)
    preamble(P, g)
    sched.run(P.bb.mf, lambda i, entry: issue_mfma(P, g, entry), K["cap"])
    sched.finish(20, epi_tail)
    return g


def main():
    g = gen(S.parse_knobs(sys.argv[2:], KNOBS))
    S.write_inc(sys.argv[1], g, "SN_X3_CHAIN", "tools/gen_x3_chain.py " + " ".join(sys.argv[2:]))
    print(S.summary_line("x3 chain", g))


if __name__ == "__main__":
    main()
