#!/usr/bin/env python3
"""Generator of the hand-scheduled trunk of the bf16 fused-MLP forward kernel (sinnerf_amd/csrc/sn_mlp_fwd_bf16_v3.hip).

The trunk = layers xyz_encoding_1..8 + xyz_encoding_final of models/nerf.py:122-140 for one wave's two 32-point tiles:
72 weight slabs (one 32-row output tile x full K each, csrc/sn_layout.h), 2176 v_mfma_f32_32x32x16_bf16.  At the bf16 MFMA
rate (32 cycles per MFMA per SIMD, one wave per SIMD) the kernel's speed is decided by WHERE the ~3 non-MFMA instructions
per MFMA sit: an instruction issued in the 32-cycle shadow of an MFMA is free, a clump of them (a 48-instruction epilogue,
an `s_waitcnt lgkmcnt(0)` behind a just-issued ds_read) is not (round 1: 49 % of peak with 4.9 instructions per MFMA, the
compiler's lgkmcnt(0) before every 4th k-step and the deferred epilogue in one block).  hipcc cannot be told where to put
instructions relative to inline-asm MFMAs, so the whole trunk is emitted as ONE asm statement whose stream is laid out here:

  * backbone: the MFMAs in execution order (slab, k-step, point tile); two accumulator sets alternate between slabs, the
    bias enters as the C operand of a slab's first k-step (no accumulator initialisation moves);
  * fillers, dealt into the gaps after each MFMA by a list scheduler (release gap, deadline, per-gap issue budget;
    tools/mfma_stream.py, shared with the other generators of such statements):
      - A-fragment ds_read_b128, PREFETCH k-steps ahead through a register ring, waited for with COUNTED lgkmcnt(N);
      - bias ds_reads of the next slab;
      - the deferred epilogue of the previous slab (cvt_pk / pk_max / accvgpr_write into the other activation set),
        two instructions per gap;
      - the weight stream: one 4 KB LDS-DMA piece at a time for the slab SIX ahead (7-slot ring with a static slot per
        slab, see N_SLOTS below), one counted-vmcnt barrier per slab;
  * hazards the compiler would pad (VALU write -> MFMA read, MFMA write -> VALU read, m0 -> LDS-DMA) are tracked on the
    emitted stream and padded with s_nop only where the schedule leaves them too close; tools/check_agpr.py re-checks
    the build.

Register plan inside the statement (physical registers, all declared as clobbers; the compiler keeps v0..v127):
  v[128:191]  accumulators  [set][point tile][16]
  v[192:207]  bias of the slab in flight (C operand of k-step 0)
  v[208:235]  A-fragment ring (prefetch + 2 entries x 4, at most 7)
  v[236:237]  LDS addresses of ring slots 3..5 and 6 (16-bit ds_read offsets reach three 20 KB slots)
  v[240:247]  epilogue temporaries (tmp_pairs of them in rotation)
  v[248:255]  sigma-head weights of the layer-8 epilogue (2 x 4, double-buffered)
  a[0:127], a[128:255]  the two activation sets (as before)

usage: gen_bf16_trunk.py out.inc [knob=value ...]     knobs: see KNOBS below (ablation builds for tools/ timing)
"""
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfma_stream as S                         # noqa: E402  (Emitter, Backbone, Scheduler, Filler, write_inc)

# ------------------------------------------------------------------------------------------------------------------
KNOBS = dict(prefetch=4,        # A-fragment prefetch distance in k-steps (ring = prefetch + 2 entries)
             cap=4.0,           # issue budget per MFMA gap (VALU / LDS instruction = 1)
             dma_cost=2.0, valu_cost=1.0, lds_cost=1.0, salu_cost=0.5,
             epi=1, dma=1, frag=1, bar=1, sigma=1,    # ablation switches (0 = leave the work out: WRONG results, timing only)
             bar_gap=3,         # the barrier sits after this MFMA of a slab
             setprio=0,
             dma_exec=0,        # experiment: 1 = every DMA runs with EXEC = %[em] (a mask the kernel supplies), WRONG results
             dma_thin=1,        # experiment: issue only every dma_thin-th piece (WRONG results)
             tmp_pairs=2,       # epilogue temporaries: pairs of v[240:247] used in rotation (2 = v[240:243]; the registers a
                                # shorter rotation does not name go back to the compiler, see the clobber list)
             store=0,           # 1 = TRAINING forward (sn_mlp_fwd_bf16_t.hip): every output tile is also written to acts[] as bf16
                                # (whole 128-byte rows, non-temporal) together with the ReLU sign words -- see STORE MODE below
             swap_rev=0,        # store mode: operand order of v_permlane32_swap_b32 (0 = vdst lanes 32..63 <-> src lanes 0..31, confirmed by
                                # the bit-identity test against the compiler-scheduled kernel on the device)
             nt=1,              # store mode: non-temporal hint on the row stores
             dma_early=0,       # 1: a slab's DMA pieces in consecutive gaps right behind the sync point (in FRONT of the slab's row stores)
             spread=1,          # store mode: row stores dealt into the next tile's epilogue (0: burst behind the odd tile)
             abl_sign4=0,       # timing experiment (WRONG results): one dwordx4 sign store per FOUR tiles instead of a dword per tile
             abl_vstore=1, abl_stage=1, abl_sign=1,   # store mode timing ablations (0 = leave out: WRONG results): the global stores, the
                                # staging round trip (swaps + LDS writes / reads + stores), the sign-word arithmetic
             f16=0,             # 1 = the SAME stream with fp16 operands (round 6, SN_DTYPE_F16): v_cvt_pk_f16_f32 / v_mfma_f32_32x32x16_f16
                                # (same issue classes and latencies; v_pk_max_i16 is a ReLU on a packed fp16 pair as on a bf16 pair)
             abl_stw=1, abl_str=1)    # ... the staging ds_write_b128s alone / the staging ds_read_b128s alone (which of the two owns the
                                # LDS bank conflicts the counters see: VERDICT r3 item 8)

STORE_KNOBS = dict(store=1, cap=6.0)            # the build of sn_mlp_fwd_bf16_t.hip (csrc/Makefile passes the same)
V_FIRST = 128                                  # first physical VGPR the statement owns (clobbers v[V_FIRST:255])
ACC = lambda st, pt: 128 + st * 32 + pt * 16   # v[128:191]
BIAS = 192                                     # v[192:207]
RING0 = 208                                    # v[208:235]: up to 7 fragment-ring entries
VA1, VA2 = 236, 237                            # LDS address registers of ring slots 3..5 / 6 (va0 + 61440, + 122880)
TMP0 = 240                                     # v[240:247]
SIGW = 248                                     # v[248:255]: two 4-register buffers
N_SLABS_TRUNK = 72
N_SLABS = 76
# Weight ring: N_SLOTS slots of SLOT_BYTES, slot of slab s = s % N_SLOTS.  76 slabs per point tile + ONE virtual empty slab
# (index 76) make the period 77 = 0 mod 7, so the slot of every slab is static across point tiles.  Slab s is staged
# DMA_DIST slabs ahead: at slab s (behind its barrier) the pieces of virtual index s + DMA_DIST are issued into slot
# (s + DMA_DIST) % 7 = (s - 1) % 7, which every wave has left.  The LDS-DMA latency under load (~1.1 us issued -> landed,
# MI355X_MICROARCH.md) is two slab times: with a 4-slot ring (distance 3) the counted vmcnt wait in front of every barrier
# stalled (measured: 13 % of the kernel); distance 6 keeps ~5 slabs = 5 us in flight.
N_SLOTS = 7
SLOT_BYTES = 20480
DMA_DIST = 6
SLOTS_PER_BASE = 3                             # ds_read offsets are 16 bit: one address VGPR per 3 slots (va0, va1, va2)

# ---- STORE MODE (training forward, bf16 state) -----------------------------------------------------------------
# Ring: 4 slots, distance 3, no virtual slab (76 = 0 mod 4): 80 KB instead of 140, which leaves room for the staging tiles.
# The slab time of the training kernel is bounded by its HBM stores, not by the MFMAs: a shorter DMA lead is affordable.
# Registers: NO extra VGPRs over the inference statement.  The packed output words of the tile being finalised are written over
# the accumulator registers they were converted from -- blocks 0 and 1 of each point tile's 16 accumulators receive
# [t0_0 t1_0 t0_2 t1_2] and [t0_1 t1_1 t0_3 t1_3], laid out so that after four v_permlane32_swap_b32 each lane half holds two
# consecutive 4-register groups = two 16-byte chunks of its point row (every conversion reads its sources before a later one
# overwrites them); they are swapped and written to LDS before slab s+2 re-uses the accumulator set.  v[240:247] two 4-register
# rows in flight (staging read -> global store), v238/v239 conversion temporaries of layer 8 (whose fp32 ReLU outputs also feed
# the sigma head), v232 the ReLU sign word, v233..v235 derived lane addresses; s[84:85] running pointer into acts[layer]
# (+ slot_rows * 512 B per layer), s[86:87] pointer to the sign-word rows.
# Staging tile of a wave (LDS, 9216 B): [point tile: 4608][b3 = tile parity: 2304][e = which of the lane's two chunks: 1152]
# [point row j: 32 B][16 * (h ^ ((j >> 2) & 1))] -- the 16-byte chunk m = 4 b3 + 2 h + e of the 128-byte row of a tile PAIR.
#   write (ds_write_b128, lane = point row): served EIGHT contiguous lanes at a time over 32 banks (128 B) -- rows j .. j+3 take the
#   four 32-byte steps of the window, rows j+4 .. j+7 the same steps with the halves swapped: 8 distinct 16-byte slots;  read
#   (ds_read_b128, lane = (g, k): row 8 i + g, chunk k; 16 lanes over 64 banks): (8 e + 2 g + (h ^ ((g >> 2) & 1))) mod 16 is a
#   bijection on every lane group.  Both conflict-free in the guide's bank model (tools/gcn_sim.py counts them; the first layout
#   swapped the halves on (j >> 3) & 1 -- conflict-free for 16-lane groups, two-way for the 8-lane groups the stores really use:
#   profiles/r04_bf16_t_bank_conflict_by_class.txt, tools/ubench/lds_b128_banks.hip).  One lane-address VGPR for the writes, one for
#   the reads (a second register still carries a copy for the odd row groups), supplied by the kernel.
ST_RO, ST_T0, ST_SB = 240, 238, 232
ST_VS, ST_STR1, ST_VSG = 233, 234, 235      # derived inside the statement: sigma-weight address, odd-row read address, sign-store offset
ST_PT, ST_B3, ST_E = 4608, 2304, 1152
ST_SGPR_ACTS, ST_SGPR_SIGN = 84, 86
ST_N_SLOTS, ST_DMA_DIST = 4, 3

def staged_at(s, store=0):
    """real slabs whose pieces are issued behind the barrier of trunk slab s (virtual indices s + DMA_DIST; slab 0 also does the
    virtual slab's duty: index 76 + DMA_DIST - 77 = 5).  Store mode: slab s + 3, always of the same point tile (the dir section
    of the kernel stages slab 75 and the next tile's slabs 0..2)."""
    if store:
        assert s + ST_DMA_DIST < N_SLABS
        return [s + ST_DMA_DIST]
    out = []
    if s == 0:
        out.append(5)
    v = s + DMA_DIST
    if v < N_SLABS:
        out.append(v)
    elif v > N_SLABS:
        out.append(v - (N_SLABS + 1) + 1000)     # slab of the NEXT point tile (tagged +1000: offsets restart at 0)
    return out

# slab kinds of the trunk (csrc/sn_layout.h): (name, k-steps from xe VGPRs, k-steps from the AGPR set)
def slab_kind(s):
    if s < 8: return ("L0", 4, 0)
    if 32 <= s < 40: return ("SKIP", 4, 16)
    return ("H", 0, 16)

def slab_k(s):           # K of every slab of the network (bytes = K * 64)
    return 64 if s < 8 else 256 if s < 32 else 320 if s < 40 else 256 if s < 72 else 288

def layer_of(s): return s // 8
# activation set read / written by a layer (sn_mlp_fwd_bf16.hip): L0 writes 0; L1 r0 w1; L2 r1 w0; L3 r0 w1; L4 r1(+xe) w0;
# L5 r0 w1; L6 r1 w0; L7 r0 w1; FIN r1 w0
READ_SET = {1: 0, 2: 1, 3: 0, 4: 1, 5: 0, 6: 1, 7: 0, 8: 1}
WRITE_SET = {0: 0, 1: 1, 2: 0, 3: 1, 4: 0, 5: 1, 6: 0, 7: 1, 8: 0}

def act_reg(st, kstep, pt): return st * 128 + (kstep * 2 + pt) * 4


def plan(K):
    """what the builders below share for one gen() call: the knobs, the backbone, ring geometry, operand-format mnemonics"""
    P = SimpleNamespace(K=K, D=K["prefetch"], R=K["prefetch"] + 2, store=K["store"])
    P.bb = S.Backbone(N_SLABS_TRUNK, lambda s: slab_kind(s)[1] + slab_kind(s)[2], 2)      # mf[i] = (slab, k-step, point tile)
    assert P.R <= 7, "fragment ring: 7 entries of registers"
    assert not P.store or P.R <= 6, "store mode keeps v232..v235 for itself"
    P.n_slots = ST_N_SLOTS if P.store else N_SLOTS
    P.dma_dist = ST_DMA_DIST if P.store else DMA_DIST
    # f16=1: the same stream with fp16 operands (same issue classes and latencies)
    P.cvt = "v_cvt_pk_f16_f32" if K["f16"] else "v_cvt_pk_bf16_f32"
    P.mfma = "v_mfma_f32_32x32x16_f16" if K["f16"] else "v_mfma_f32_32x32x16_bf16"
    return P


def ring(P, kidx): return RING0 + 4 * (kidx % P.R)       # kidx = global k-step counter over the trunk

def frag_read(P, kidx):
    s, ks = P.bb.kstep_list[kidx]
    slot, r = s % P.n_slots, ring(P, kidx)
    base = ("%[va0]", "v%d" % VA1, "v%d" % VA2)[slot // SLOTS_PER_BASE]
    return "ds_read_b128 v[%d:%d], %s offset:%d" % (r, r + 3, base, (slot % SLOTS_PER_BASE) * SLOT_BYTES + ks * 1024)

def bias_read(s, q):
    return "ds_read_b128 v[%d:%d], %%[vb] offset:%d" % (BIAS + 4 * q, BIAS + 4 * q + 3, s * 128 + q * 16)


def add_fragments(P, sched):
    """A fragments.  The first D k-steps of the trunk are loaded in the preamble (slab 0 is resident: the previous tile's / the
    prologue's barrier guaranteed it)"""
    K, D, R, first, idx_of, ksl = P.K, P.D, P.R, P.bb.first, P.bb.idx_of, P.bb.kstep_list
    for kidx in range(D, len(ksl) if K["frag"] else 0):
        s, ks = ksl[kidx]
        # release: after the previous user of this ring entry has issued (k-step kidx - R, its pt-1 MFMA) and, when the
        # fragment belongs to a LATER slab than the one executing at that point, after that slab's barrier
        prev_user = idx_of[ksl[kidx - R] + (1,)] if kidx - R >= 0 else -1
        rel = max(prev_user, idx_of[ksl[kidx - D] + (0,)])                                # ideal gap: D k-steps ahead
        bar_ok = first[s - 1] + K["bar_gap"] if s > 0 else -1                            # barrier(s-1) makes slab s visible
        rel = max(rel, bar_ok + 1) if K["bar"] else rel
        sched.add(S.Filler(frag_read(P, kidx), K["lds_cost"], rel, idx_of[(s, ks, 0)] - 1, "ds_read", tag=("frag", kidx)))


def add_bias(P, sched):
    """bias of slab s: 4 x ds_read_b128 into v[192:207]; free once k-step 0 of slab s-1 has issued (+2 MFMAs)"""
    first = P.bb.first
    for s in range(1, N_SLABS_TRUNK):
        rel = first[s - 1] + 3
        dl = first[s] - 1
        # spread over the last gaps of the previous slab
        span = max(1, (first[s] - 1) - rel)
        for q in range(4):
            r = max(rel, first[s] - 10 + 2 * q) if span > 10 else rel
            sched.add(S.Filler(bias_read(s, q), P.K["lds_cost"], r, dl, "ds_read", tag=("bias", s)))


# ---- epilogue of slab s, run inside slab s+1 (the last one is flushed after the backbone): items as class Scheduler takes them ----
def store_epilogue(P, s):
    K, cvt = P.K, P.cvt
    L, t = layer_of(s), s % 8
    W, st = WRITE_SET[L], s & 1
    sigma, copy = L == 7, L == 8
    PKR = lambda pt, n: ACC(st, pt) + n              # packed word n of the point tile: over accumulator blocks 0, 1
    # block i of a point tile -> its two packed words; after the swaps PK[0:3] = chunk e=0, PK[4:7] = chunk e=1 of the lane
    slot_of = {0: (0, 1), 2: (2, 3), 1: (4, 5), 3: (6, 7)}
    sigw = lambda i: SIGW + 4 * (i & 1)
    items = []
    def sig_load(i):
        items.append(("ds_read", "ds_read_b128 v[%d:%d], v%d offset:%d" % (sigw(i), sigw(i) + 3, ST_VS, (16 * t + 4 * i) * 4), (), ("sigw", s, i), "acc"))
    step = [0]
    def sign(word):
        if step[0] == 0:
            items.append(("valu", "v_and_b32 v%d, %%[sm], v%d" % (ST_SB, word), (ST_SB,), None, "acc"))
        else:
            items.append(("valu", "v_lshrrev_b32 v%d, 1, v%d" % (ST_SB, ST_SB), (ST_SB,), None, "acc"))
            items.append(("valu", "v_and_or_b32 v%d, v%d, %%[sm], v%d" % (ST_SB, word, ST_SB), (ST_SB,), None, "acc"))
        step[0] += 1
    def block(pt, i):
        a = ACC(st, pt) + 4 * i
        t0, t1 = PKR(pt, slot_of[i][0]), PKR(pt, slot_of[i][1])
        q = 2 * i
        r0 = act_reg(W, 2 * t + (q >> 2), pt) + (q & 3)
        if sigma:
            # layer 8: signs from the packed raw values, sigma head from the fp32 ReLU outputs (nerf.py:136, as in inference),
            # ReLU of the packed pair lands in the point tile's packed-word registers (pk_max(cvt(x), 0) == cvt(max(x, 0)))
            c0, c1 = ST_T0, ST_T0 + 1
            items.append(("valu", "%s v%d, v%d, v%d" % (cvt, c0, a, a + 1), (c0,), None, "acc"))
            items.append(("valu", "%s v%d, v%d, v%d" % (cvt, c1, a + 2, a + 3), (c1,), None, "acc"))
            sign(c0); sign(c1)
            for e in range(4):
                items.append(("valu", "v_max_f32 v%d, 0, v%d" % (a + e, a + e), (a + e,), None, "acc"))
            for e in range(4):
                items.append(("valu", "v_fmac_f32 %%[sg%d], v%d, v%d" % (pt, sigw(i) + e, a + e), (), ("sigw", s, i), "acc"))
            items.append(("valu", "v_pk_max_i16 v%d, v%d, 0" % (t0, c0), (t0,), None, "acc"))
            items.append(("valu", "v_pk_max_i16 v%d, v%d, 0" % (t1, c1), (t1,), None, "acc"))
        else:
            items.append(("valu", "%s v%d, v%d, v%d" % (cvt, t0, a, a + 1), (t0,), None, "acc"))
            items.append(("valu", "%s v%d, v%d, v%d" % (cvt, t1, a + 2, a + 3), (t1,), None, "acc"))
            if not copy:
                sign(t0)
                items.append(("valu", "v_pk_max_i16 v%d, v%d, 0" % (t0, t0), (t0,), None, "acc"))
                sign(t1)
                items.append(("valu", "v_pk_max_i16 v%d, v%d, 0" % (t1, t1), (t1,), None, "acc"))
        items.append(("valu", "v_accvgpr_write_b32 a%d, v%d" % (r0, t0), (("a", r0),), None, "acc"))
        items.append(("valu", "v_accvgpr_write_b32 a%d, v%d" % (r0 + 1, t1), (("a", r0 + 1),), None, "acc"))
    fin = []                                             # packed words -> staging planes (both point tiles), behind everything else
    def finish_pt(pt):
        pairs = [(PKR(pt, 0), PKR(pt, 2)), (PKR(pt, 1), PKR(pt, 3)), (PKR(pt, 4), PKR(pt, 6)), (PKR(pt, 5), PKR(pt, 7))]
        for x, y in pairs:
            if K["swap_rev"]:
                x, y = y, x
            fin.append(("swap", "v_permlane32_swap_b32 v%d, v%d" % (x, y), (x, y), None, "acc", (x, y)))
        for e in range(2):
            off = pt * ST_PT + (t & 1) * ST_B3 + e * ST_E
            if K["abl_stw"]:
                fin.append(("ds_write", "ds_write_b128 %%[stw], v[%d:%d] offset:%d" % (PKR(pt, 4 * e), PKR(pt, 4 * e) + 3, off), (), None, "acc"))
    if sigma:                                            # q outermost, both point tiles share a quad's sigma weights
        sig_load(0); sig_load(1)
        for i in range(4):
            for pt in range(2):
                block(pt, i)
            if i + 2 < 4:
                sig_load(i + 2)
    else:                                                # point tile outermost: the sign-word step order of the chain
        for pt in range(2):
            for i in range(4):
                block(pt, i)
    finish_pt(0); finish_pt(1)
    if not copy and K["abl_sign4"]:
        if t % 4 == 3:
            items.append(("vstore", "global_store_dwordx4 v%d, v[%d:%d], s[%d:%d] nt" % (ST_VSG, ST_SB, ST_SB + 3, ST_SGPR_SIGN, ST_SGPR_SIGN + 1), (), None, "post",
                          (ST_SGPR_SIGN, ST_SGPR_SIGN + 1)))
    elif not copy:                                       # the tile's ReLU sign word: 256 contiguous bytes per wave
        items.append(("vstore", "global_store_dword v%d, v%d, s[%d:%d] nt" % (ST_VSG, ST_SB, ST_SGPR_SIGN, ST_SGPR_SIGN + 1), (), None, "post",
                      (ST_SGPR_SIGN, ST_SGPR_SIGN + 1)))
        items.append(("valu", "v_add_u32 v%d, 512, v%d" % (ST_VSG, ST_VSG), (ST_VSG,), None, "post"))
    readout = store_readout(K, s) if t & 1 else []
    if not K["abl_stage"]:
        fin, readout = [], []
    if not K["abl_sign"]:
        items = [it for it in items if ("v%d" % ST_SB) not in it[1]]
    return items, fin, readout


def store_readout(K, s):
    """store mode, odd tile: tiles t-1, t of both point tiles leave the staging planes as whole 128-byte rows"""
    t = s % 8
    tp = t >> 1
    items = []
    rows = [(pt, i) for pt in range(2) for i in range(4)]
    def rd(n):
        pt, i = rows[n]
        ro = ST_RO + 4 * (n % 2)
        src = "v%d" % ST_STR1 if (i & 1) else "%[str0]"
        if K["abl_str"]:
            items.append(("ds_read", "ds_read_b128 v[%d:%d], %s offset:%d" % (ro, ro + 3, src, pt * ST_PT + 256 * i), (), ("ro", s, n), "post"))
    def stw(n):
        ro = ST_RO + 4 * (n % 2)
        rokey = ("ro", s, n) if K["abl_str"] else None
        if K["abl_vstore"]:
            items.append(("vstore", "global_store_dwordx4 %%[vo], v[%d:%d], s[%d:%d] offset:%d%s" % (ro, ro + 3, ST_SGPR_ACTS, ST_SGPR_ACTS + 1, 128 * tp, " nt" if K["nt"] else ""),
                          (), rokey, "post", (ST_SGPR_ACTS, ST_SGPR_ACTS + 1)))
        else:                                        # timing ablation: the staged row is still waited for, nothing leaves
            items.append(("valu", "s_nop 0", (), rokey, "post"))
        if n < 7:
            items.append(("valu", "v_add_u32 %[vo], 4096, %[vo]", ("vo",), None, "post"))
        else:
            items.append(("valu", "v_subrev_u32 %[vo], 28672, %[vo]", ("vo",), None, "post"))
    rd(0); rd(1)
    for n in range(8):
        stw(n)
        if n + 2 < 8:
            rd(n + 2)
    if t == 7:                                       # next layer: acts[L + 1]
        items.append(("salu", "s_add_u32 s%d, s%d, %%[srlo]" % (ST_SGPR_ACTS, ST_SGPR_ACTS), (ST_SGPR_ACTS,), None, "post"))
        items.append(("salu", "s_addc_u32 s%d, s%d, %%[srhi]" % (ST_SGPR_ACTS + 1, ST_SGPR_ACTS + 1), (ST_SGPR_ACTS + 1,), None, "post"))
    return items


def store_flat(P, s):
    """epilogue stream of slab s in store mode.  The row stores of a finished tile PAIR are not issued as a burst behind the odd
    tile's epilogue: they are dealt evenly into the NEXT (even) tile's epilogue, in front of its staging writes (which re-use
    the planes) -- one store per ~4 MFMAs instead of eight within a few gaps.  A wave whose store cannot issue (the CU's address
    path is full) cannot issue its MFMAs either: without the staging round trip the kernel ran 0.51 ms, with it 0.72."""
    items, fin, readout = store_epilogue(P, s)
    prev = store_epilogue(P, s - 1)[2] if (s > 0 and P.K["spread"]) else []
    out = S.interleave(items, prev) + fin
    if not P.K["spread"] or s == N_SLABS_TRUNK - 1:
        out += readout                                   # (the last pair of the trunk: behind the backbone)
    return out


def plain_epilogue(P, s):
    K, cvt = P.K, P.cvt
    L, t = layer_of(s), s % 8
    W = WRITE_SET[L]
    st = s & 1
    sigma = (L == 7) and K["sigma"]
    copy = (L == 8)
    groups = []
    sigw = lambda i: SIGW + 4 * (i & 1)
    def sig_load(i):                                 # sigma-head weights of quad i of this tile (both point tiles share them)
        return [("ds_read", "ds_read_b128 v[%d:%d], %%[vs] offset:%d" % (sigw(i), sigw(i) + 3, (16 * t + 4 * i) * 4), (), ("sigw", s, i), "acc")]
    if sigma:
        groups.append(sig_load(0)); groups.append(sig_load(1))
    for i in range(4):
        for pt in range(2):
            a = ACC(st, pt) + 4 * i
            t0, t1 = TMP0 + 2 * ((2 * i + pt) % K["tmp_pairs"]), TMP0 + 2 * ((2 * i + pt) % K["tmp_pairs"]) + 1
            q = 2 * i
            r0 = act_reg(W, 2 * t + (q >> 2), pt) + (q & 3)
            ins = []
            if sigma:
                for e in range(4):
                    ins.append(("valu", "v_max_f32 v%d, 0, v%d" % (a + e, a + e), (a + e,), None, "acc"))
                for e in range(4):
                    ins.append(("valu", "v_fmac_f32 %%[sg%d], v%d, v%d" % (pt, sigw(i) + e, a + e), (), ("sigw", s, i), "acc"))
            ins.append(("valu", "%s v%d, v%d, v%d" % (cvt, t0, a, a + 1), (t0,), None, "acc"))
            ins.append(("valu", "%s v%d, v%d, v%d" % (cvt, t1, a + 2, a + 3), (t1,), None, "acc"))
            if not sigma and not copy:
                ins.append(("valu", "v_pk_max_i16 v%d, v%d, 0" % (t0, t0), (t0,), None, "acc"))
                ins.append(("valu", "v_pk_max_i16 v%d, v%d, 0" % (t1, t1), (t1,), None, "acc"))
            ins.append(("valu", "v_accvgpr_write_b32 a%d, v%d" % (r0, t0), (("a", r0),), None, "acc"))
            ins.append(("valu", "v_accvgpr_write_b32 a%d, v%d" % (r0 + 1, t1), (("a", r0 + 1),), None, "acc"))
            groups.append(ins)
        if sigma and i + 2 < 4:                      # the buffer quad i used is free once its fmacs have issued (in order)
            groups.append(sig_load(i + 2))
    return [x for grp in groups for x in grp]


def add_epilogues(P, sched):
    """Returns the last slab's epilogue (flushed behind the backbone).  The activation registers have a deadline of their own: the
    next layer reads k-steps 2t, 2t+1 of the written set.  Only the LAST tile of a layer is read soon (k-steps 14, 15 of the next
    layer's first slab); everything else only has the accumulator deadline."""
    if not P.K["epi"]:
        return []
    def handover(s):
        L, t = layer_of(s), s % 8
        if t == 7 and L + 1 <= 8:
            nxt = 8 * (L + 1)
            return P.bb.idx_of[(nxt, (4 if nxt == 32 else 0) + 14, 0)]       # skip layer: 4 xe k-steps come first
    flat_of = (lambda s: store_flat(P, s)) if P.store else (lambda s: plain_epilogue(P, s))
    return sched.add_deferred_epilogues(P.bb, flat_of, 1, handover, program_order=P.store)


def add_weight_stream(P, sched):
    """barrier + weight stream: at slab s, barrier (slab s+1 visible), then the DMA pieces of staged_at(s)"""
    K, first = P.K, P.bb.first
    for s in range(N_SLABS_TRUNK):
        b = first[s] + K["bar_gap"]
        if K["bar"]:
            sched.add(S.Filler("", 0.5, b, b, "bar", tag=s + 1))
        if not K["dma"]:
            continue
        plist = []                                    # (lds byte offset, goff bump, tag)
        for tgt in staged_at(s, P.store):
            real = tgt - 1000 if tgt >= 1000 else tgt
            nbytes = slab_k(real) * 64
            slot = real % P.n_slots
            for p in range(-(-nbytes // 4096)):
                bump = min(4096, nbytes - p * 4096)
                if tgt >= 1000 and real == 0 and p == 0:
                    bump = None                       # the stream wraps: goff restarts at tid*16 (+4096 behind this piece)
                plist.append((slot * SLOT_BYTES + p * 4096, bump, s + P.dma_dist if (tgt != 5 or P.store) else 5))
        gaps_avail = max(1, first[s + 1] - first[s] - K["bar_gap"] - 3)
        stride = 1 if K["dma_early"] else max(1, gaps_avail // max(1, len(plist)))
        dl = first[s + 1] - 1
        for p, (lds_off, bump, tag) in enumerate(plist):
            rel = min(b + 1 + p * stride, dl)
            if bump is None:                          # back to the start of the blob: minus the whole weight stream (76 slabs)
                sched.weight_stream_piece("s_add_u32 m0, %%[wv1k], %d" % lds_off, rel, dl, tag,
                                          rewind=sum(slab_k(x) * 64 for x in range(N_SLABS)))
            else:
                sched.weight_stream_piece("s_add_u32 m0, %%[wv1k], %d" % lds_off, rel, dl, tag, bump=bump)


def preamble(P, g):
    """address registers, first D fragments + bias of slab 0"""
    g.emit("v_add_u32 v%d, %d, %%[va0]" % (VA1, SLOTS_PER_BASE * SLOT_BYTES))
    if not P.store:
        g.emit("v_add_u32 v%d, %d, %%[va0]" % (VA2, 2 * SLOTS_PER_BASE * SLOT_BYTES))
    else:                                                # running pointers of the statement (physical SGPRs, declared as clobbers)
        for dst, src in ((ST_SGPR_ACTS, "aplo"), (ST_SGPR_ACTS + 1, "aphi"), (ST_SGPR_SIGN, "sglo"), (ST_SGPR_SIGN + 1, "sghi")):
            g.salu_mov(dst, "%%[%s]" % src)
        # lane addresses derived from the kernel's: vb = TAIL + 64 h -> sigma weights at TAIL + 4 (BIAS_FLOATS + 128 h) = 8 vb - 7 TAIL
        # + 4 BIAS_FLOATS (%[vsk] = that constant); the odd-row staging read address = a copy of str0; the sign-store offset = lane * 4
        g.emit("v_lshl_add_u32 v%d, %%[vb], 3, %%[vsk]" % ST_VS)
        g.emit("v_mov_b32 v%d, %%[str0]" % ST_STR1)
        g.emit("v_lshrrev_b32 v%d, 2, %%[va0]" % ST_VSG)
    for q in range(4):
        g.ds_read(bias_read(0, q), ("bias", 0))
    if P.K["frag"]:
        for kidx in range(P.D):
            g.ds_read(frag_read(P, kidx), ("frag", kidx))
    else:
        g.ds_read("ds_read_b128 v[%d:%d], %%[va0] offset:0" % (RING0, RING0 + 3), ("frag", 0))


def issue_mfma(P, g, entry):
    s, ks, pt = entry
    frag = P.K["frag"]
    kidx = P.bb.gk[(s, ks)]
    nx = slab_kind(s)[1]
    need = {("frag", kidx if frag else 0)}
    if ks == 0:
        need.add(("bias", s))
    g.wait_lgkm(need)
    a_reg = ring(P, kidx) if frag else RING0
    d = ACC(s & 1, pt)
    c = BIAS if ks == 0 else d                           # the bias enters as the C operand of the slab's first k-step
    if ks < nx:
        b_txt = "%%[xe%d]" % (ks * 2 + pt)
    else:
        b0 = act_reg(READ_SET[layer_of(s)], ks - nx, pt)
        b_txt = "a[%d:%d]" % (b0, b0 + 3)
        g.pad_valu_to_mfma([("a", b0 + e) for e in range(4)])
    g.mfma("%s v[%d:%d], v[%d:%d], %s, v[%d:%d]" % (P.mfma, d, d + 15, a_reg, a_reg + 3, b_txt, c, c + 15))


def gen(knobs):
    K, P = knobs, plan(knobs)
    # LDS-DMA pieces that may be in flight on entry: at most the single pieces of slabs 1..4, issued by the previous tile's
    # dir_encoding section / the prologue; store mode (distance 3): slabs 1, 2
    g = S.Emitter([1, 2] if K["store"] else [1, 2, 3, 4], dma_thin=K["dma_thin"], dma_exec=K["dma_exec"])
    sched = S.Scheduler(g, K["dma_cost"], K["valu_cost"], K["lds_cost"], K["salu_cost"])
    add_fragments(P, sched)
    add_bias(P, sched)
    epi_tail = add_epilogues(P, sched)
    add_weight_stream(P, sched)
    if K["setprio"]:
        g.emit("s_setprio %d" % K["setprio"])
    preamble(P, g)
    sched.run(P.bb.mf, lambda i, entry: issue_mfma(P, g, entry), K["cap"])
    sched.finish(12, epi_tail)                           # MFMA results: 11 wait states
    g.nop(2)                                             # accvgpr_write -> the compiler's first dir_encoding MFMA
    if K["setprio"]:
        g.emit("s_setprio 0")
    return g


def main():
    g = gen(S.parse_knobs(sys.argv[2:], KNOBS))
    S.write_inc(sys.argv[1], g, "SN_BF16_TRUNK", "tools/gen_bf16_trunk.py " + " ".join(sys.argv[2:]), v_first=V_FIRST)
    print(S.summary_line("trunk", g))


if __name__ == "__main__":
    main()
