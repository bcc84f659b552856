#!/usr/bin/env python3
"""Generator of the hand-scheduled slab loop of the bf16-state backward chain (sinnerf_amd/csrc/sn_mlp_bwd_bf16_t.hip).

The chain = input-gradient propagation g_x = W^T g_y, g_y = g_h (.) act'(.) through dir_encoding^T, xyz_encoding_final^T and
xyz_encoding_8..2^T -- what torch autograd derives from models/nerf.py:122-148 -- for one wave's two 32-point tiles: the 72
transposed weight slabs of csrc/sn_layout.h ("Backward-chain blob, bf16 operands"), 2176 v_mfma_f32_32x32x16_bf16.  Like the
training forward (tools/gen_bf16_trunk.py store=1) it is emitted as ONE asm statement whose instruction stream is laid out by
the same list scheduler (tools/mfma_stream.py): MFMAs back to back, everything else dealt into their shadows with counted waits.

Per output tile (slab s, tile t of a layer) the deferred epilogue, run inside slab s+1:
  * xyz_encoding_final^T only: the sigma head's term x += sigma.weight[f] * g_sigma (nerf.py:136) on the fp32 accumulators;
  * conversion to packed bf16 pairs IN PLACE over accumulator blocks 0 / 1 of the point tile (as in the forward's store mode);
  * ReLU mask from the SIGN WORD the training forward left for this (layer, tile): shift the pair's two bits down, isolate
    (c01 = 0x00010001), subtract 1 per half -> 0xffff where the forward value was positive, AND (csrc/sn_mlp_bf16.h
    epi_relu_bits; step order: point tile outermost, except layer 8 whose forward epilogue runs quad outermost);
  * hand-over to the next transposed layer: v_accvgpr_write into the other activation set;
  * the masked pairs ARE the pre-activation gradients g_y the weight-gradient kernels read: four v_permlane32_swap_b32, two
    conflict-free ds_write_b128 into the wave's staging planes, every second tile eight ds_read_b128 + global_store_dwordx4 of
    whole 128-byte rows of G[slot] (non-temporal).
Sign words: one dword per lane and tile, ALL 64 of a point tile loaded at the top of the statement into a register file
(v[64:127]) behind which the eight short dir_encoding^T slabs run before the first mask is needed.  Loads inside the slab loop --
even a layer ahead of their use -- sit in the same issue-ordered vmcnt queue as the weight DMA: every barrier's counted wait for
the next slab's pieces then also waits for the youngest sign-word load in front of them, an HBM read queued behind 4 TB/s of row
stores (measured: the chain lost 0.23 ms to its stores, the forward -- no loads in its trunk -- 0.13; TCP->TCC write latency is
only ~320 cycles, so it is not the stores themselves that hold the queue).

Weight ring: 4 slots of 16 KB (the widest transposed slab), slab s in slot s % 4 (72 = 0 mod 4: static), staged 3 slabs ahead,
slabs 69..71 stage the next point tile's slabs 0..2 (the stream wraps).  No bias: the first k-step of a slab takes C = 0.

Register plan inside the statement (v[128:255] declared as clobbers where named):
  v[128:191] accumulators [set][point tile][16]      v[192:199] two 4-register rows in flight (staging read -> global store)
  v[200:207] sigma^T weights (2 x 4, double-buffered)  v[208:231] A-fragment ring (6 entries)
  v232/v233 mask temporaries   v234 sign-load offset   v235 odd-row staging read address   v[64:127] sign-word file [acts slot][tile]
  s[84:85] running pointer into G[slot] (- slot_rows * 512 B per layer), s[86:87] pointer to the sign-word rows

usage: gen_bf16_chain.py out.inc [knob=value ...]
"""
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfma_stream as S                         # noqa: E402  (Emitter, Backbone, Scheduler, Filler, write_inc)
import gen_bf16_trunk as T                      # noqa: E402  (accumulator / AGPR numbering, staging-plane constants)

KNOBS = dict(prefetch=4, cap=6.0, dma_cost=2.0, valu_cost=1.0, lds_cost=1.0, salu_cost=0.5, bar_gap=3,
             abl_vstore=1, abl_stage=1, abl_mask=1)           # timing ablations (0 = leave out: WRONG results)

N_SLABS = 72
N_SLOTS, SLOT_BYTES, DMA_DIST = 4, 16384, 3
RO, SIGT, M0, VSG, STR1, SWF = 192, 200, 232, 234, 235, 64
SGPR_G, SGPR_SIGN = 84, 86
ACC, RING0, act_reg = T.ACC, T.RING0, T.act_reg
ST_PT, ST_B3, ST_E = T.ST_PT, T.ST_B3, T.ST_E


def nk_of(s): return 8 if s < 8 else 16
def layer_of(s): return s // 8                # 0 dir_encoding^T, 1 xyz_encoding_final^T, 2.. xyz_encoding_{li+1}^T with li = 9 - layer
def slab_bytes(s): return nk_of(s) * 1024
def read_set(L): return 0 if L == 0 else 1 if L == 1 else (0 if (9 - L) & 1 else 1)
def write_set(L): return 1 - read_set(L)
def out_slot(L): return 8 if L == 0 else 7 if L == 1 else 8 - L       # G slot the layer writes = acts slot of its ReLU mask
TOTAL_BYTES = sum(slab_bytes(s) for s in range(N_SLABS))
# sign words: the word of (chain layer L >= 1, tile t) = acts slot 8 - L ... v[SWF + 8 slot + t], loaded in the preamble
def swreg(L, t): return SWF + 8 * out_slot(L) + t


def plan(K):
    P = SimpleNamespace(K=K, D=K["prefetch"], R=K["prefetch"] + 2)
    assert P.R <= 6
    P.bb = S.Backbone(N_SLABS, nk_of, 2)             # mf[i] = (slab, k-step, point tile)
    return P


def frag_read(P, kidx):
    s, ks = P.bb.kstep_list[kidx]
    r = RING0 + 4 * (kidx % P.R)
    return "ds_read_b128 v[%d:%d], %%[va0] offset:%d" % (r, r + 3, (s % N_SLOTS) * SLOT_BYTES + ks * 1024)


def add_fragments(P, sched):
    """A fragments (first D k-steps in the preamble: slab 0 is resident); release as in gen_bf16_trunk.py"""
    K, D, R, first, idx_of, ksl = P.K, P.D, P.R, P.bb.first, P.bb.idx_of, P.bb.kstep_list
    for kidx in range(D, len(ksl)):
        s, ks = ksl[kidx]
        prev_user = idx_of[ksl[kidx - R] + (1,)] if kidx - R >= 0 else -1
        rel = max(prev_user, idx_of[ksl[kidx - D] + (0,)])
        bar_ok = first[s - 1] + K["bar_gap"] if s > 0 else -1
        rel = max(rel, bar_ok + 1)
        sched.add(S.Filler(frag_read(P, kidx), K["lds_cost"], rel, idx_of[(s, ks, 0)] - 1, "ds_read", tag=("frag", kidx)))


def epilogue(K, s):
    """epilogue of slab s (run inside slab s+1): (block items, staging writes, row stores of the tile PAIR)"""
    L, t = layer_of(s), s % 8
    W, st = write_set(L), s & 1
    copy, sig = L == 0, L == 1
    PKR = lambda pt, n: ACC(st, pt) + n
    slot_of = {0: (0, 1), 2: (2, 3), 1: (4, 5), 3: (6, 7)}
    sigt = lambda i: SIGT + 4 * (i & 1)
    items, fin = [], []
    def sig_load(i):
        items.append(("ds_read", "ds_read_b128 v[%d:%d], %%[vst] offset:%d" % (sigt(i), sigt(i) + 3, (16 * t + 4 * i) * 4), (), ("sigt", s, i), "acc"))
    def block(pt, i):
        a = ACC(st, pt) + 4 * i
        t0, t1 = PKR(pt, slot_of[i][0]), PKR(pt, slot_of[i][1])
        q = 2 * i
        r0 = act_reg(W, 2 * t + (q >> 2), pt) + (q & 3)
        if sig:                                         # + sigma.weight[f] * g_sigma (nerf.py:136), fp32
            for e in range(4):
                items.append(("valu", "v_fmac_f32 v%d, v%d, %%[gs%d]" % (a + e, sigt(i) + e, pt), (a + e,), ("sigt", s, i), "acc"))
        items.append(("valu", "v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (t0, a, a + 1), (t0,), None, "acc"))
        items.append(("valu", "v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (t1, a + 2, a + 3), (t1,), None, "acc"))
        if not copy and K["abl_mask"]:
            j0 = (4 * i + 2 * pt) if sig else (8 * pt + 2 * i)
            sw = swreg(L, t)
            items.append(("valu", "v_lshrrev_b32 v%d, %d, v%d" % (M0, j0, sw), (M0,), ("vm", ("sw", out_slot(L), t)), "acc"))
            items.append(("valu", "v_lshrrev_b32 v%d, %d, v%d" % (M0 + 1, j0 + 1, sw), (M0 + 1,), None, "acc"))
            items.append(("valu", "v_and_b32 v%d, %%[c01], v%d" % (M0, M0), (M0,), None, "acc"))
            items.append(("valu", "v_and_b32 v%d, %%[c01], v%d" % (M0 + 1, M0 + 1), (M0 + 1,), None, "acc"))
            items.append(("valu", "v_pk_sub_u16 v%d, v%d, %%[c01]" % (M0, M0), (M0,), None, "acc"))
            items.append(("valu", "v_pk_sub_u16 v%d, v%d, %%[c01]" % (M0 + 1, M0 + 1), (M0 + 1,), None, "acc"))
            items.append(("valu", "v_and_b32 v%d, v%d, v%d" % (t0, t0, M0), (t0,), None, "acc"))
            items.append(("valu", "v_and_b32 v%d, v%d, v%d" % (t1, t1, M0 + 1), (t1,), None, "acc"))
        items.append(("valu", "v_accvgpr_write_b32 a%d, v%d" % (r0, t0), (("a", r0),), None, "acc"))
        items.append(("valu", "v_accvgpr_write_b32 a%d, v%d" % (r0 + 1, t1), (("a", r0 + 1),), None, "acc"))
    def finish_pt(pt):                                  # packed words -> staging planes, behind the block items of BOTH point tiles
        for x, y in [(PKR(pt, 0), PKR(pt, 2)), (PKR(pt, 1), PKR(pt, 3)), (PKR(pt, 4), PKR(pt, 6)), (PKR(pt, 5), PKR(pt, 7))]:
            fin.append(("swap", "v_permlane32_swap_b32 v%d, v%d" % (x, y), (x, y), None, "acc", (x, y)))
        for e in range(2):
            off = pt * ST_PT + (t & 1) * ST_B3 + e * ST_E
            fin.append(("ds_write", "ds_write_b128 %%[stw], v[%d:%d] offset:%d" % (PKR(pt, 4 * e), PKR(pt, 4 * e) + 3, off), (), None, "acc"))
    if sig:
        sig_load(0); sig_load(1)
        for i in range(4):
            for pt in range(2):
                block(pt, i)
            if i + 2 < 4:
                sig_load(i + 2)
    else:
        for pt in range(2):
            for i in range(4):
                block(pt, i)
    finish_pt(0); finish_pt(1)
    readout = readout_rows(K, s) if t & 1 else []
    if not K["abl_stage"]:
        fin, readout = [], []
    return items, fin, readout


def readout_rows(K, s):
    """odd tile: tiles t-1, t of both point tiles leave the staging planes as whole 128-byte rows of G[slot]"""
    t = s % 8
    tp = t >> 1
    items = []
    rows = [(pt, i) for pt in range(2) for i in range(4)]
    def rd(n):
        pt, i = rows[n]
        ro = RO + 4 * (n % 2)
        src = "v%d" % STR1 if (i & 1) else "%[str0]"
        items.append(("ds_read", "ds_read_b128 v[%d:%d], %s offset:%d" % (ro, ro + 3, src, pt * ST_PT + 256 * i), (), ("ro", s, n), "post"))
    def stw(n):
        ro = RO + 4 * (n % 2)
        if K["abl_vstore"]:
            items.append(("vstore", "global_store_dwordx4 %%[vo], v[%d:%d], s[%d:%d] offset:%d nt" % (ro, ro + 3, SGPR_G, SGPR_G + 1, 128 * tp),
                          (), ("ro", s, n), "post", (SGPR_G, SGPR_G + 1)))
        else:                                            # timing ablation: the staged row is still waited for, nothing leaves
            items.append(("valu", "s_nop 0", (), ("ro", s, n), "post"))
        items.append(("valu", ("v_add_u32 %[vo], 4096, %[vo]" if n < 7 else "v_subrev_u32 %[vo], 28672, %[vo]"), ("vo",), None, "post"))
    rd(0); rd(1)
    for n in range(8):
        stw(n)
        if n + 2 < 8:
            rd(n + 2)
    if t == 7:                                       # next layer: G[slot - 1]
        items.append(("salu", "s_sub_u32 s%d, s%d, %%[srlo]" % (SGPR_G, SGPR_G), (SGPR_G,), None, "post"))
        items.append(("salu", "s_subb_u32 s%d, s%d, %%[srhi]" % (SGPR_G + 1, SGPR_G + 1), (SGPR_G + 1,), None, "post"))
    return items


def flat_of(K, s):
    """block items of tile s with the PREVIOUS tile pair's row stores dealt evenly between them, then the staging writes (which
    re-use the planes those stores read): see store_flat in gen_bf16_trunk.py"""
    items, fin, readout = epilogue(K, s)
    prev = epilogue(K, s - 1)[2] if s > 0 else []
    out = S.interleave(items, prev) + fin
    if s == N_SLABS - 1:
        out += readout
    return out


def add_weight_stream(P, sched):
    """barrier + weight stream: at slab s (behind the sync point) the pieces of slab s + 3 (the stream wraps to the next point tile)"""
    first = P.bb.first
    for s in range(N_SLABS):
        b = first[s] + P.K["bar_gap"]
        sched.add(S.Filler("", 0.5, b, b, "bar", tag=s + 1))
        v = s + DMA_DIST
        real = v % N_SLABS
        pieces = slab_bytes(real) // 4096
        gaps_avail = max(1, first[s + 1] - first[s] - P.K["bar_gap"] - 3)
        stride = max(1, gaps_avail // max(1, pieces))
        dl = first[s + 1] - 1
        for p in range(pieces):
            wrap = v >= N_SLABS and real == 0 and p == 0                  # back to the start of the blob
            sched.weight_stream_piece("s_add_u32 m0, %%[wv1k], %d" % ((real % N_SLOTS) * SLOT_BYTES + p * 4096),
                                      min(b + 1 + p * stride, dl), dl, v, rewind=TOTAL_BYTES if wrap else None)


def preamble(P, g):
    for dst, src in ((SGPR_G, "gplo"), (SGPR_G + 1, "gphi"), (SGPR_SIGN, "sglo"), (SGPR_SIGN + 1, "sghi")):
        g.salu_mov(dst, "%%[%s]" % src)
    g.emit("v_mov_b32 v%d, %%[str0]" % STR1)
    g.emit("v_lshrrev_b32 v%d, 2, %%[va0]" % VSG)
    if P.K["abl_mask"]:
        g.nop(4)                                                                  # SALU write of the sign pointer -> VMEM address
        for slot in range(8):                                                    # rows p_wave + 8 slot + t, 512 B each
            for t in range(8):
                g.emit("global_load_dword v%d, v%d, s[%d:%d] offset:%d nt" % (SWF + 8 * slot + t, VSG, SGPR_SIGN, SGPR_SIGN + 1, 512 * t))
                g.vm.append(("sw", slot, t))
            if slot < 7:
                g.emit("v_add_u32 v%d, 4096, v%d" % (VSG, VSG))
    for kidx in range(P.D):
        g.ds_read(frag_read(P, kidx), ("frag", kidx))


def issue_mfma(P, g, entry):
    s, ks, pt = entry
    kidx = P.bb.gk[(s, ks)]
    g.wait_lgkm({("frag", kidx)})
    a_reg = RING0 + 4 * (kidx % P.R)
    d = ACC(s & 1, pt)
    b0 = act_reg(read_set(layer_of(s)), ks, pt)
    g.pad_valu_to_mfma([("a", b0 + e) for e in range(4)])
    c_txt = "0" if ks == 0 else "v[%d:%d]" % (d, d + 15)
    g.mfma("v_mfma_f32_32x32x16_bf16 v[%d:%d], v[%d:%d], a[%d:%d], %s" % (d, d + 15, a_reg, a_reg + 3, b0, b0 + 3, c_txt))


def gen(knobs):
    K, P = knobs, plan(knobs)
    g = S.Emitter([1, 1, 2, 2])                   # entry: at most the two pieces each of slabs 1, 2 in flight
    sched = S.Scheduler(g, K["dma_cost"], K["valu_cost"], K["lds_cost"], K["salu_cost"])
    add_fragments(P, sched)
    def handover(s):                              # the next layer's first slab reads k-steps 14, 15 of the written set last
        if s % 8 == 7:
            return P.bb.idx_of[(s + 1, nk_of(s + 1) - 2, 0)]
    epi_tail = sched.add_deferred_epilogues(P.bb, lambda s: flat_of(K, s), 1, handover)
    add_weight_stream(P, sched)
    preamble(P, g)
    sched.run(P.bb.mf, lambda i, entry: issue_mfma(P, g, entry), K["cap"])
    sched.finish(12, epi_tail)
    g.nop(2)
    return g


def main():
    g = gen(S.parse_knobs(sys.argv[2:], KNOBS))
    S.write_inc(sys.argv[1], g, "SN_BF16_CHAIN", "tools/gen_bf16_chain.py " + " ".join(sys.argv[2:]), v_first=64)
    print(S.summary_line("chain", g))


if __name__ == "__main__":
    main()
